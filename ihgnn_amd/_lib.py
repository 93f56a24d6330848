"""ctypes binding of libihgnn_hip.so (C ABI: include/ihgnn_hip.h).

There is exactly one implementation of the hot path - the HIP library.  If it cannot be loaded the
first call raises; nothing in this package falls back to PyTorch or CPU code.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_void_p
from typing import Optional

# torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be in the process
# BEFORE libihgnn_hip.so is opened, so that the library's DT_NEEDED entry resolves to that same runtime: kernels are
# then enqueued on torch's streams, against torch's allocations, by one runtime.  Two runtimes in one process see
# "no ROCm-capable device".
import torch  # noqa: F401  (side effect: loads the HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
# IHGNN_HIP_LIBRARY points at another build of the same ABI (A/B timing of kernel variants); default: the in-tree library
LIB_PATH = os.environ.get('IHGNN_HIP_LIBRARY') or os.path.join(_HERE, 'csrc', 'libihgnn_hip.so')

ABI_VERSION = 37

OK, ERR_INVALID, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3
SCALE_NONE, SCALE_MULTIPLY, SCALE_DIVIDE = 0, 1, 2
SCALE_ACCUMULATE = 0x100      # OR-ed into the mode of ihg_node_segment_sum: out += instead of out =
SRC_READ_ONCE = 0x400         # OR-ed into the mode of ihg_node_segment_sum: every source row of this launch is read exactly once (non-temporal loads)
SRC_SCALE_IN_ENTRIES = 0x800  # OR-ed into the mode of ihg_node_segment_sum: entry_scale already holds src_scale[ids] (x the entry weights); src_scale serves the row's own term only

_i64p, _i32p, _f32p = POINTER(c_int64), POINTER(c_int32), POINTER(c_float)

# The ranking entry points' argument groups (include/ihgnn_hip.h), from which their six signatures below are composed:
_SCORE_HEAD = [c_void_p, c_int64, c_int32, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]      # features, ld, dim, query_row0, item_row0, n_items, item_bias, users, queries
_SEARCH_SOURCES = [c_void_p, c_int64, c_int32, c_void_p]                                               # query_rows, ld_q, q_dim, item_mask
_EXCLUSION = [c_void_p, c_void_p, c_void_p, c_int64]                                                   # excl_ptr, excl_items, excl_row, n_excl_rows
_CANDIDATES = [c_void_p, c_void_p, c_void_p, c_int64, c_int64]                                         # cand_ptr, cand_items, cand_row, n_cand_rows, total
_RANKED = [c_float, c_int64, c_int32, c_void_p, c_void_p]                                              # lambda_muq, n_pairs, k, top_scores, top_items
_WORKSPACE = [c_void_p, c_int64]
_DEEP_TAIL = [c_int32, c_void_p, c_void_p]                                                             # cosine, passes, stream

# name -> (restype, argtypes); mirrors include/ihgnn_hip.h line by line.  Device pointers travel as
# c_void_p (tensor.data_ptr()); host-side builders take real typed pointers.
SIGNATURES = {
    'ihg_abi_version': (c_int32, []),
    'ihg_ablation_build': (c_int32, []),
    'ihg_last_error_string': (c_char_p, []),
    'ihg_build_csr': (ctypes.c_int, [_i64p, c_int64, c_int64, c_int64, c_int64, _i32p, _i32p, _i32p, _f32p]),
    'ihg_parse_search_logs': (ctypes.c_int, [c_char_p, _i64p, _i64p, _i64p, _i64p, c_int64, _i64p, c_int64, _i64p]),
    'ihg_read_graph_info': (ctypes.c_int, [c_char_p, _i64p]),
    'ihg_read_query_bags': (ctypes.c_int, [c_char_p, _i64p, _i64p, _i64p, c_int64, _i64p, c_int64]),
    'ihg_build_log_hypergraph': (ctypes.c_int, [_i64p, _i64p, c_int64, c_int64, c_int64, c_int64, _i32p, _i32p, _f32p, _f32p, _i32p, _i32p, _f32p, _f32p,
                                                _i64p, _i64p]),
    'ihg_build_pair_csr': (ctypes.c_int, [_i64p, c_int64, c_int64, c_int64, c_int64, c_int32, c_int32, _i32p, _i32p, _f32p, _f32p,
                                          c_int64, _i64p]),
    'ihg_transpose_csr': (ctypes.c_int, [_i32p, _i32p, c_int64, c_int64, _i32p, _i32p]),
    'ihg_merge_id_lists': (ctypes.c_int, [_i32p, _i32p, _f32p, c_int64, _i32p, _i32p, _f32p, _i64p]),
    'ihg_unique_triples': (ctypes.c_int, [_i64p, c_int64, c_int64, c_int64, c_int64, _i64p, _f32p, _i32p, _i64p]),
    'ihg_edge_gather_sum': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                           c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_edge_gather_sum_planes_supported': (c_int32, [c_int32, c_int64]),
    'ihg_edge_gather_sum_planes': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_segment_sum': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                            c_void_p, c_int64, c_int64, c_int32, c_int32,
                                            c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ihg_bag_mean_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                        c_int64, c_int32, c_void_p]),
    'ihg_bag_mean_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                        c_int64, c_int32, c_void_p]),
    'ihg_interact_fwd_workspace_bytes': (c_int64, [c_int64, c_int32, c_int32]),
    'ihg_interact_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32,
                                        c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_interact_bwd_workspace_bytes': (c_int64, [c_int64, c_int32, c_int32]),
    'ihg_interact_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64,
                                        c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_interact_bwd_user_reduced_supported': (c_int32, [c_int32, c_int32, c_int64]),
    'ihg_interact_bwd_user_reduced': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                                     c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_interact_bwd_user_reduced_planes_supported': (c_int32, [c_int32, c_int32, c_int64]),
    'ihg_interact_bwd_user_reduced_planes': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                                            c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_interact_bwd_gathered_supported': (c_int32, [c_int32, c_int32, c_int64, c_int64]),
    'ihg_interact_bwd_gathered': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                                 c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_interact_bwd_gathered_first_order_supported': (c_int32, [c_int32, c_int32, c_int64, c_int64]),
    'ihg_interact_bwd_gathered_first_order': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                                             c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32,
                                                             c_void_p]),
    'ihg_node_pair_sums': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32,
                                          c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'ihg_node_interact_fwd_supported': (c_int32, [c_int32, c_int32, c_int64, c_int64, c_int64]),
    'ihg_node_interact_fwd_workspace_bytes': (c_int64, [c_int32]),
    'ihg_node_interact_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, _i64p,
                                             c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_interact_bwd_weight_supported': (c_int32, [c_int32, c_int32, c_int64, c_int64, c_int64]),
    'ihg_node_interact_bwd_weight_workspace_bytes': (c_int64, [c_int32, c_int32]),
    'ihg_node_interact_bwd_weight': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, _i64p,
                                                    c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_linear_workspace_bytes': (c_int64, [c_int32]),
    'ihg_rows_linear_act_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_rows_linear_act_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                               c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_linear_bwd_accumulates': (c_int32, [c_int32, c_int64, c_int64, c_int64]),
    'ihg_node_linear_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int32, c_int64, _i64p,
                                           c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_linear_bwd_input': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, _i64p, c_void_p, c_int64,
                                                 c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_linear_bwd_weight': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, _i64p, c_void_p, c_int64, c_int64,
                                                  c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32,
                                                  c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_hem_score_fwd': (ctypes.c_int, [POINTER(c_void_p), c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_float,
                                         c_void_p, c_int64, c_void_p]),
    'ihg_hem_score_bwd': (ctypes.c_int, [POINTER(c_void_p), c_int32, c_int64, c_int32, c_void_p, c_void_p, c_float, c_float,
                                         c_void_p, c_int64, c_int64, c_void_p]),
    'ihg_bce_with_logits': (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'ihg_ranking_loss': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    'ihg_hard_negative_loss': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ihg_batch_scatter_workspace_bytes': (c_int64, [c_int64]),
    'ihg_batch_scatter_max_rows': (c_int32, []),
    'ihg_batch_scatter_add': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int64,
                                             c_void_p, c_int64, c_int64, c_void_p]),
    'ihg_compose_first_order_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    'ihg_compose_first_order_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                   c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    'ihg_adam_step': (ctypes.c_int, [c_void_p, c_int32, c_float, c_float, c_float, c_float, c_float, c_int64, c_void_p]),
    'ihg_adam_step_device_scalars': (ctypes.c_int, [c_void_p, c_int32, c_float, c_float, c_float, c_float, c_void_p, c_void_p]),
    'ihg_grad_sqnorm_workspace_bytes': (c_int64, [c_void_p, c_int32]),
    'ihg_grad_sqnorm': (ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    'ihg_clip_record': (ctypes.c_int, [c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    'ihg_adam_step_clipped': (ctypes.c_int, [c_void_p, c_int32, c_float, c_float, c_float, c_float, c_float, c_int64, c_void_p, c_void_p]),
    'ihg_adam_step_clipped_device_scalars': (ctypes.c_int, [c_void_p, c_int32, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    'ihg_batch_combine': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    'ihg_sample_negatives': (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    'ihg_sample_pool': (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    'ihg_sample_pool_excluding': (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                 c_void_p]),
    'ihg_sample_pool_weighted': (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                                c_void_p, c_void_p]),
    'ihg_device_batch': (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                        c_void_p, c_void_p]),
    'ihg_score_topk_max_dim': (c_int32, []),
    'ihg_score_topk_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32]),
    'ihg_score_topk': (ctypes.c_int, _SCORE_HEAD + _RANKED + _WORKSPACE + [c_void_p]),
    'ihg_batch_rows_add': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                          c_void_p]),
    # typed rows: the first row of every node type at its own address (host arrays of three device pointers)
    'ihg_node_linear_typed_supported': (c_int32, [c_int32, c_int64, c_int64]),
    'ihg_node_linear_fwd_typed': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int32, c_int64, _i64p, c_void_p, c_int64,
                                                 c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_node_linear_bwd_weight_typed': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, _i64p, c_void_p, c_int64, c_int64, c_void_p, c_int32, c_int64,
                                                        c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_hem_score_fwd_typed0': (ctypes.c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64, _i64p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                                c_void_p, c_int64, c_void_p]),
    'ihg_hem_score_bwd_typed0': (ctypes.c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64, _i64p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                                c_void_p, c_int64, c_int64, c_void_p]),
    'ihg_batch_rows_put': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int64, _i64p, c_int32, c_void_p]),
    # the cosine head (Gs.Prediction.use_cosine_similarity): the _typed0 shape plus the per-row stats, and ihg_score_topk's signature
    'ihg_hem_cosine_fwd': (ctypes.c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64, _i64p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                          c_void_p, c_void_p, c_int64, c_void_p]),
    'ihg_hem_cosine_bwd': (ctypes.c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64, _i64p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                          c_void_p, c_int64, c_int64, c_void_p]),
    'ihg_score_topk_cosine': (ctypes.c_int, _SCORE_HEAD + _RANKED + _WORKSPACE + [c_void_p]),
    # ranking deeper than ten (csrc/eval.hip): ihg_score_topk's arguments, then the head, then the optional per-pair pass counts
    'ihg_score_topk_max_k': (c_int32, []),
    'ihg_score_topk_deep_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    'ihg_score_topk_deep': (ctypes.c_int, _SCORE_HEAD + _RANKED + _WORKSPACE + _DEEP_TAIL),
    # answering a search (csrc/eval.hip): ihg_score_topk_deep with (queries | query_rows, ld_q, q_dim), the candidate mask words and users < 0 = no user
    'ihg_search_topk_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    'ihg_search_topk': (ctypes.c_int, _SCORE_HEAD + _SEARCH_SOURCES + _RANKED + _WORKSPACE + _DEEP_TAIL),
    # ... that leaves out a list of items per pair: ihg_search_topk with (excl_ptr, excl_items, excl_row, n_excl_rows) after the mask
    'ihg_search_topk_excluding_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    'ihg_search_topk_excluding': (ctypes.c_int, _SCORE_HEAD + _SEARCH_SOURCES + _EXCLUSION + _RANKED + _WORKSPACE + _DEEP_TAIL),
    # re-ranking a shortlist per search (csrc/candidates.hip): ihg_search_topk_excluding's sources, then (cand_ptr, cand_items, cand_row, n_cand_rows, total), and all_scores
    'ihg_search_candidates_max_dim': (c_int32, []),
    'ihg_search_candidates_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    'ihg_search_candidates': (ctypes.c_int, _SCORE_HEAD + _SEARCH_SOURCES + _EXCLUSION + _CANDIDATES + _RANKED + [c_void_p] + _WORKSPACE + _DEEP_TAIL),
    'ihg_zero_floats': (ctypes.c_int, [c_void_p, c_int64, c_void_p]),
    'ihg_mark_rows': (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    'ihg_batch_node_rows': (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    'ihg_zero_rows': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p]),
    # GAT attention over the pairwise graph (csrc/gat.hip)
    'ihg_gat_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    'ihg_gat_attention_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                             c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int64, c_void_p]),
    'ihg_gat_scores_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                          c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int64, c_void_p]),
    'ihg_gat_symmetrize': (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    'ihg_gat_finish_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64, c_void_p,
                                          c_void_p, c_void_p, c_int64, c_void_p]),
    # phase-2 attention of IHGNNLayer over the node <- hyperedge incidence (csrc/phase2.hip)
    'ihg_phase2_workspace_bytes': (c_int64, [c_int64, c_int64, c_int64, c_int32, c_int32]),
    'ihg_phase2_attention_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    'ihg_phase2_scores_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    'ihg_phase2_edges_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64, c_void_p]),
    'ihg_phase2_add_rows': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_phase2_finish_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    # the Srrl baseline (csrc/srrl.hip): a source of the block is (base, ld, width, idx, rep)
    'ihg_cat_linear_max_width': (c_int32, []),
    'ihg_cat_linear_workspace_bytes': (c_int64, [c_int64, c_int32, c_int32]),
    'ihg_cat_linear_fwd': (ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                                          c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    'ihg_cat_linear_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64,
                                          c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                          c_void_p, c_int64, c_void_p]),
    'ihg_rows_dot_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_rows_dot_bwd': (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ihg_kg_loss': (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    'ihg_rows_topk': (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    # the GRU query encoder (csrc/recurrent.hip)
    'ihg_gru_workspace_bytes': (c_int64, [c_int64, c_int64, c_int32]),
    'ihg_gru_saved_bytes': (c_int64, [c_int64, c_int32]),
    'ihg_gru_fwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                   c_void_p, c_int64, c_int32, c_void_p]),
    'ihg_gru_bwd': (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
}
ACT_NONE, ACT_LEAKY_RELU = 0, 3
LOSS_KINDS = {'bpr': 1, 'softmax': 2}      # IHG_LOSS_BPR / IHG_LOSS_SOFTMAX
HARD_NEGATIVE_KINDS = {'bce': 0, **LOSS_KINDS}      # ihg_hard_negative_loss also takes IHG_LOSS_BCE
POOL_MAX = 256                             # candidates per positive: ihg_sample_pool's m, ihg_hard_negative_loss's pool

_lib: Optional[ctypes.CDLL] = None


class IhgnnHipError(RuntimeError):
    """A libihgnn_hip entry point returned a non-zero status."""


def load() -> ctypes.CDLL:
    """Bind the library (once).  Raises if it is missing, stale in ABI, or lacks a declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IhgnnHipError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'(hipcc --offload-arch=gfx950).  ihgnn_amd has no CPU or PyTorch fallback for this path.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise IhgnnHipError(f'{LIB_PATH} does not export {name} (declared in include/ihgnn_hip.h)') from exc
        fn.restype, fn.argtypes = restype, argtypes
    got = lib.ihg_abi_version()
    if got != ABI_VERSION:
        raise IhgnnHipError(f'{LIB_PATH} has ABI version {got}, this package needs {ABI_VERSION}: rebuild it')
    if lib.ihg_ablation_build() and os.environ.get('IHG_ALLOW_ABLATION_BUILD') != '1':
        raise IhgnnHipError(f'{LIB_PATH} is an ablation build (csrc/ablate.hpp: a kernel with part of its work removed, wrong results on purpose); '
                            'only the timing tools load one (IHG_ALLOW_ABLATION_BUILD=1)')
    _lib = lib
    return lib


def last_error() -> str:
    return load().ihg_last_error_string().decode('utf-8', 'replace')


def check(status: int, what: str) -> None:
    if status != OK:
        raise IhgnnHipError(f'{what} failed with status {status}: {last_error()}')
