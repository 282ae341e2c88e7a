"""ctypes binding of libtgnx.so (the C ABI declared in include/tgnx.h).

The product path has no CPU fallback: if the library is missing or no HIP
device is visible, every op raises.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TGNX_LIB") or os.path.join(_HERE, "libtgnx.so")

c_i32, c_i64, c_u64, c_sz, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p
P = c_vp  # every device pointer crosses as void*

# name -> (restype, argtypes); must match include/tgnx.h
SIGNATURES = {
    "tgnx_version": (ctypes.c_int, []),
    "tgnx_last_error": (ctypes.c_char_p, []),
    "tgnx_ring_reset": (ctypes.c_int, [P, P, c_i64, c_i32, c_vp]),
    "tgnx_ring_sample_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_ring_sample": (ctypes.c_int, [P, P, P, c_i64, c_i32, P, c_i64, P, P, P, P, P, c_i64, c_i64, P, P, c_sz,
                                        c_vp]),
    "tgnx_ring_insert_max_batch": (ctypes.c_int, []),
    "tgnx_ring_insert": (ctypes.c_int, [P, P, P, c_i64, c_i32, P, P, P, c_i64, c_i64, P, c_vp]),
    "tgnx_neg_sample": (ctypes.c_int, [P, c_i64, P, c_i64, c_u64, c_u64, P, c_vp]),
    "tgnx_block_ids_host": (ctypes.c_int, [P, P, c_i64, c_i64, P]),
    "tgnx_probe_enable": (ctypes.c_int, [c_i32]),
    "tgnx_probe_read": (ctypes.c_int, [P, P]),
    "tgnx_stamps_set": (ctypes.c_int, [P, ctypes.c_uint32]),
    "tgnx_stamps_count": (c_i64, []),
    "tgnx_tgnn_param_layout": (ctypes.c_int, [P, P]),
    "tgnx_tgnn_ws_bytes": (c_sz, [P]),
    "tgnx_tgnn_ws_misc_offset": (c_sz, [P]),
    "tgnx_tgn_param_layout": (ctypes.c_int, [P, P]),
    "tgnx_tgn_ws_bytes": (c_sz, [P]),
    "tgnx_tgn_store_words": (c_sz, [P]),
    "tgnx_tgn_reset_state": (ctypes.c_int, [P, P, c_vp]),
    "tgnx_tgn_plan_table_bytes": (c_sz, [P, c_i64, c_i64, c_i64]),
    "tgnx_tgn_plan_table": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, P, c_sz, c_vp]),
    "tgnx_tgn_plan_table_release": (ctypes.c_int, [P]),
    "tgnx_tgn_train_fwd_bwd": (ctypes.c_int, [P, P, c_i32, c_i32, c_vp]),
    "tgnx_tgn_train_update": (ctypes.c_int, [P, P, c_vp]),
    "tgnx_tgn_train_step": (ctypes.c_int, [P, P, c_i32, c_i32, c_vp]),
    "tgnx_tgn_train_step_resident": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_i32, c_vp]),
    "tgnx_tgn_train_step_pipelined": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_u64, c_i32, c_i32, c_vp]),
    "tgnx_tgn_train_step_pp": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_u64, c_i32, c_i32, c_i32, c_vp]),
    "tgnx_tgn_train_fwd_bwd_resident": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_i32, c_vp]),
    "tgnx_tgn_train_fwd_bwd_pipelined": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_i32, c_i32,
                                                         c_vp]),
    "tgnx_tgn_apply_rows_update": (ctypes.c_int, [P, P, P, c_i64, c_vp]),
    "tgnx_tgn_train_fwd_bwd_split": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_i32, c_i32, c_vp]),
    "tgnx_tgn_train_fwd_bwd_pp": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_i32, c_i32, c_i32,
                                                  c_i32, P, c_i64, c_vp]),
    "tgnx_tgn_scan_next": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_vp]),
    "tgnx_tgn_step_plan": (ctypes.c_int, [P, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, P]),
    "tgnx_tgn_eval_step": (ctypes.c_int, [P, P, c_i32, c_vp]),
    "tgnx_tgn_eval_step_resident": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_i32, c_u64, P, c_vp]),
    "tgnx_tgn_embed_max_nodes": (c_i64, [P]),
    "tgnx_tgn_embed": (ctypes.c_int, [P, P, P, c_i64, P, P, c_vp]),
    "tgnx_tgn_explain": (ctypes.c_int, [P, P, P, c_i64, c_i32, P, P, P, P, P, P, P, c_vp]),
    "tgnx_tgn_observe_step": (ctypes.c_int, [P, P, c_vp]),
    # the embedding table's stale-row bookkeeping (tgnx_embtab.hip) and its refresh
    "tgnx_embtab_touch": (ctypes.c_int, [P, P, c_i64, c_i64, P, c_vp]),
    "tgnx_embtab_expand": (ctypes.c_int, [P, P, P, c_vp]),
    "tgnx_embtab_list_ws_bytes": (c_sz, [c_i64]),
    "tgnx_embtab_list": (ctypes.c_int, [P, c_i64, c_i32, P, P, P, c_sz, c_vp]),
    "tgnx_tgn_embed_into": (ctypes.c_int, [P, P, P, c_i64, P, c_vp]),
    "tgnx_tgn_compact_ws_bytes": (c_sz, [P, c_i64]),
    "tgnx_tgn_compact_plan": (ctypes.c_int, [P, P, c_i64, c_i64, P, c_sz, c_vp]),
    "tgnx_tgn_compact_apply": (ctypes.c_int, [P, P, c_i64, c_i64, P, P, P, P, P, P, c_i64, P, c_sz, c_vp]),
    "tgnx_tgn_grow_nodes": (ctypes.c_int, [P, P, c_i64, c_i64, P, P, c_vp]),
    "tgnx_tgn_grow_store": (ctypes.c_int, [P, P, c_i64, P, P, c_vp]),
    "tgnx_tgn_forget_ws_bytes": (c_sz, [P]),
    "tgnx_tgn_forget_plan": (ctypes.c_int, [P, P, c_i64, P, c_i64, P, c_sz, c_vp]),
    "tgnx_tgn_forget_apply": (ctypes.c_int, [P, P, c_i64, P, c_sz, P, c_vp]),
    "tgnx_ring_forget": (ctypes.c_int, [P, P, P, P, c_i64, c_i64, c_i32, P, c_i64, P, c_sz, c_vp]),
    "tgnx_tgn_flush": (ctypes.c_int, [P, P, P, ctypes.c_size_t, c_vp]),
    "tgnx_tgn_flush_scratch_bytes": (ctypes.c_size_t, [P]),
    "tgnx_tgn_apply_rows": (ctypes.c_int, [P, P, P, c_i64, c_vp]),
    "tgnx_tcsr_build_ws_bytes": (c_sz, [c_i64, c_i32]),
    "tgnx_tcsr_build": (ctypes.c_int, [P, P, P, c_i64, c_i64, c_i32, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_tcsr_sample": (ctypes.c_int, [P, P, P, P, c_i64, c_i32, P, c_i64, c_i32, P, c_i64, P, P, P, P, P, c_vp]),
    # pair index and hist_rnd evaluation negatives (tgnx_negs.hip)
    "tgnx_pair_index_build_ws_bytes": (c_sz, [c_i64]),
    "tgnx_pair_index_build": (ctypes.c_int, [P, P, c_i64, c_i64, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_pair_index_contains": (ctypes.c_int, [P, P, P, c_i64, P, P, c_i64, P, c_i64, P, c_vp]),
    "tgnx_negs_hist_rnd_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_negs_hist_rnd": (ctypes.c_int, [P, P, P, c_i32, c_i64, c_i64, c_i64, c_i32, c_i32, c_i64, P, P, P, c_i64,
                                          c_i64, P, c_i64, c_u64, c_i64, P, P, P, P, c_sz, c_vp]),
    # live pair set (tgnx_pairset.hip)
    "tgnx_pairset_bytes": (c_sz, [c_i64]),
    "tgnx_pairset_init": (ctypes.c_int, [P, c_i64, c_vp]),
    "tgnx_pairset_insert": (ctypes.c_int, [P, c_i64, P, P, P, c_i64, c_i64, P, c_vp]),
    "tgnx_pairset_import": (ctypes.c_int, [P, c_i64, P, P, P, P, c_i64, c_i64, P, c_vp]),
    "tgnx_pairset_lookup": (ctypes.c_int, [P, c_i64, c_i64, P, P, c_i64, P, ctypes.c_float, P, P, P, P, c_vp]),
    "tgnx_pairset_select_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_pairset_select_count": (ctypes.c_int, [P, c_i64, c_i64, P, c_i64, P, c_i64, P, ctypes.c_float, P, P, c_sz,
                                                 c_vp]),
    "tgnx_pairset_select_fill": (ctypes.c_int, [P, c_i64, c_i64, P, c_i64, P, c_i64, P, ctypes.c_float, P, c_i64, P,
                                                c_sz, c_vp]),
    "tgnx_pairset_rehash": (ctypes.c_int, [P, c_i64, P, c_i64, P, c_i64, P, c_vp]),
    "tgnx_pairset_export": (ctypes.c_int, [P, c_i64, P, P, P, P, c_i64, P, c_vp]),
    "tgnx_gemm_f32_ws_bytes": (c_sz, [c_i64, c_i64, c_i64]),
    "tgnx_gemm_f32": (ctypes.c_int, [c_i64, c_i64, c_i64, P, c_i64, c_i32, P, c_i64, c_i32, P, c_i64, P, c_i32, P, c_sz,
                                     c_vp]),
    # per-operator entry points (tgnx_ops.hip)
    "tgnx_msg_agg_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_msg_agg": (ctypes.c_int, [c_i32, P, c_i64, c_i64, P, P, c_i32, c_i64, P, P, P, P, c_sz, c_vp]),
    "tgnx_memory_cell_ws_bytes": (c_sz, [c_i64, c_i64, c_i64]),
    "tgnx_memory_cell": (ctypes.c_int, [c_i32, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_link_predictor_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64]),
    "tgnx_link_predictor": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_i32, P, P, c_sz,
                                           c_vp]),
    "tgnx_link_predictor_topk_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i32]),
    "tgnx_link_predictor_topk": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_i32, c_i32, P, P, P,
                                                P, c_sz, c_vp]),
    "tgnx_link_predictor_topk_filtered_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i32]),
    "tgnx_link_predictor_topk_filtered": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_i32, c_i32,
                                                         P, P, P, P, c_i64, P, P, P, P, c_sz, c_vp]),
    "tgnx_link_predictor_topk_lists_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i32, c_i64]),
    "tgnx_link_predictor_topk_lists": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_i32, c_i32,
                                                      P, P, c_i64, c_i64, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_link_predictor_rank_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64]),
    "tgnx_link_predictor_rank": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_i64, P, P, P, P, P,
                                                c_i64, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_link_predictor_loo_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64]),
    "tgnx_link_predictor_loo": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, P, P, P, P, P,
                                               P, P, P, c_sz, c_vp]),
    "tgnx_embed_knn_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i32]),
    "tgnx_embed_knn": (ctypes.c_int, [c_i64, c_i64, c_i64, P, P, c_i32, c_i32, P, P, P, P, c_i64, P, P, P, P, c_sz,
                                      c_vp]),
    "tgnx_edge_attn_fwd": (ctypes.c_int, [c_i64, c_i64, c_i32, c_i32, P, P, P, P, P, P, P, c_vp]),
    "tgnx_edge_attn_bwd": (ctypes.c_int, [c_i64, c_i64, c_i32, c_i32, P, P, P, P, P, P, P, P, P, P, P, c_vp]),
    # ... p, seed, stream_id, dst_key, edge_key, stream
    "tgnx_edge_attn_drop_fwd": (ctypes.c_int, [c_i64, c_i64, c_i32, c_i32, P, P, P, P, P, P, P, ctypes.c_float,
                                               c_u64, c_u64, P, P, c_vp]),
    "tgnx_edge_attn_drop_bwd": (ctypes.c_int, [c_i64, c_i64, c_i32, c_i32, P, P, P, P, P, P, P, P, P, P, P,
                                               ctypes.c_float, c_u64, c_u64, P, P, c_vp]),
    # per-operator backward (tgnx_ops_bwd.hip)
    "tgnx_col_sum_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_col_sum": (ctypes.c_int, [c_i64, c_i64, P, c_i64, P, P, c_sz, c_vp]),
    "tgnx_memory_cell_bwd_ws_bytes": (c_sz, [c_i64, c_i64, c_i64]),
    "tgnx_memory_cell_bwd": (ctypes.c_int, [c_i32, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_sz,
                                            c_vp]),
    "tgnx_link_predictor_bwd_ws_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64]),
    "tgnx_link_predictor_bwd": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, P, c_i32, P, P, P, P,
                                               P, P, P, P, P, c_sz, c_vp]),
    "tgnx_time_encode": (ctypes.c_int, [c_i64, c_i64, P, P, P, P, c_vp]),
    "tgnx_time_encode_bwd_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_time_encode_bwd": (ctypes.c_int, [c_i64, c_i64, P, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_time_embedding": (ctypes.c_int, [c_i64, c_i64, P, P, P, P, P, c_vp]),
    "tgnx_time_embedding_bwd_ws_bytes": (c_sz, [c_i64, c_i64]),
    "tgnx_time_embedding_bwd": (ctypes.c_int, [c_i64, c_i64, P, P, P, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_msg_agg_last_bwd": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, P, c_vp]),
    "tgnx_msg_agg_mean_bwd_ws_bytes": (c_sz, [c_i64]),
    "tgnx_msg_agg_mean_bwd": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, P, P, P, c_sz, c_vp]),
    # node property prediction (tgnx_nodeprop.hip)
    "tgnx_node_predictor_ws_bytes": (c_sz, [c_i64, c_i64, c_i64]),
    "tgnx_node_predictor": (ctypes.c_int, [c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_node_predictor_bwd_ws_bytes": (c_sz, [c_i64, c_i64, c_i64]),
    "tgnx_node_predictor_bwd": (ctypes.c_int, [c_i64, c_i64, c_i64, P, P, P, P, P, P, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_node_loss_ndcg": (ctypes.c_int, [c_i64, c_i64, c_i32, P, P, P, ctypes.c_float, P, P, P, P, c_vp]),
    # device message store (tgnx_memstore.hip)
    "tgnx_memstore_put": (ctypes.c_int, [P, P, P, P, c_i64, c_i64, P, P, c_i64, c_i64, c_i64, P, P, P, P, P, P, P,
                                         c_vp]),
    "tgnx_memstore_gather_ws_bytes": (c_sz, [c_i64]),
    "tgnx_memstore_count": (ctypes.c_int, [P, c_i64, P, c_i64, P, P, P, c_sz, c_vp]),
    "tgnx_memstore_gather": (ctypes.c_int, [P, c_i64, P, P, c_i64, P, c_i64, c_i64, c_i64, P, P, P, P, P, c_sz, c_vp]),
    "tgnx_memstore_build_msg": (ctypes.c_int, [P, c_i64, c_i64, P, P, P, P, c_i64, c_i64, c_i64, c_i64, c_i64, P, P, P,
                                               P, P, c_i64, P, P, P, c_i64, c_i32, P, P, c_vp]),
    "tgnx_tgnn_advance": (ctypes.c_int, [P, c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64,
                                         c_i32, c_vp]),
    "tgnx_tgnn_train_fwd_bwd": (ctypes.c_int, [P, P, c_i32, c_i32, c_vp]),
    "tgnx_tgnn_train_fwd_bwd_resident": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_i32, c_i32, c_u64, c_i32, c_vp]),
    "tgnx_tgnn_train_step_resident": (ctypes.c_int, [P, P, c_i64, c_i64, c_i64, c_u64, c_i32, c_vp]),
    "tgnx_tgnn_apply_pending": (ctypes.c_int, [P, P, c_vp]),
    "tgnx_tgnn_train_update": (ctypes.c_int, [P, P, c_vp]),
    "tgnx_tgnn_eval_step": (ctypes.c_int, [P, P, c_i32, c_i32, c_vp]),
    # test hooks over the GEMM core (tgnx_gemm_probe.hip)
    "tgnx_gemm_probe_ws_bytes": (c_sz, [c_i32, c_i32, c_i64, c_i64, c_i64]),
    "tgnx_gemm_probe": (ctypes.c_int, [c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, P, P, c_i64, c_i32, P, P, c_i64, c_i32,
                                       P, c_i64, P, c_i32, P, c_sz, c_vp]),
    "tgnx_gemm_probe_batch_ws_bytes": (c_sz, [P]),
    "tgnx_gemm_probe_batch": (ctypes.c_int, [P, c_i32, P, c_i32, c_i32, P, P, P, c_sz, c_vp]),
}
# a train step's launches in order (TGNX_TGN_STEP_LABELS of include/tgnx.h): tgnx_tgn_step_plan's records
STEP_LABELS = ("tgn_mark", "tgn_scan", "tgn_gather", "tgn_agg_emit", "tgn_gru_edge", "tgn_proj", "tgn_attn_fwd", "tgn_proj2",
               "tgn_attn_fwd2", "tgn_pred_train", "tgn_emb_update", "tgn_emb_update_gru", "tgn_attn_bwd2", "tgn_kv_reduce2",
               "tgn_dh1", "tgn_attn_bwd", "tgn_wgrad_dz0", "tgn_wgrad3", "tgn_scan_early", "tgn_fixup_update", "tgn_scan_next")


class TgnLaunch(ctypes.Structure):                                      # tgnx_tgn_launch
    _fields_ = [(n, c_i32) for n in ("label", "issued", "grid", "block", "lds", "kernel")]


GEMM_PROBE_CFGS = {"G32": 0, "G32L": 1, "GW": 2, "G64": 3, "GD": 4}    # TGNX_GEMM_PROBE_* of include/tgnx.h


class GemmProbeJob(ctypes.Structure):                                   # tgnx_gemm_probe_job
    _fields_ = [("M", c_i64), ("N", c_i64), ("K", c_i64), ("A", P), ("lda", c_i64), ("B", P), ("ldb", c_i64),
                ("C", P), ("ldc", c_i64), ("bias", P), ("accumulate", c_i32), ("smax", c_i32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"tgnx: {LIB_PATH} is missing — build it with `make -C tgb-tgn-dgl_amd` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("TGNX_LIB") and not hasattr(L, name):
                continue    # (an older library selected for a same-box A/B: entry points it predates stay unbound)
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def call(name: str, *args) -> None:
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        msg = lib().tgnx_last_error().decode(errors="replace")
        raise RuntimeError(f"{name} failed ({rc}): {msg}")


def ptr(t: torch.Tensor | None):
    return c_vp(0 if t is None else t.data_ptr())


def stream(device: torch.device | None = None):
    return c_vp(torch.cuda.current_stream(device).cuda_stream)


def require_device(device) -> torch.device:
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("tgnx runs only on a HIP device (MI355X); got device=%r, "
                           "torch.cuda.is_available()=%s" % (device, torch.cuda.is_available()))
    lib()
    return dev
