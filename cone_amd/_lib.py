"""ctypes binding of libcone_hip.so (include/cone_hip.h).

This is the whole FFI surface: every product code path goes through these calls, and a
missing / unbuilt library is a hard error (there is no CPU fallback anywhere in cone_amd).
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcone_hip.so")

MAX_LAYERS = 8
MAX_PROJ = 3

c_float_p = C.c_void_p  # device pointers travel as integers


class Linear(C.Structure):
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p)]


class LNorm(C.Structure):
    _fields_ = [("g", C.c_void_p), ("b", C.c_void_p)]


class Mha(C.Structure):
    _fields_ = [("in_proj_w", C.c_void_p), ("in_proj_b", C.c_void_p), ("out_proj", Linear)]


class EncLayer(C.Structure):
    _fields_ = [("self_attn", Mha), ("linear1", Linear), ("linear2", Linear), ("norm1", LNorm),
                ("norm2", LNorm)]


class DecLayer(C.Structure):
    _fields_ = [("self_attn", Mha), ("cross_attn", Mha), ("linear1", Linear), ("linear2", Linear),
                ("norm1", LNorm), ("norm2", LNorm), ("norm3", LNorm)]


class Weights(C.Structure):
    _fields_ = [
        ("hidden_dim", C.c_int32), ("nheads", C.c_int32), ("dim_ff", C.c_int32), ("enc_layers", C.c_int32),
        ("dec_layers", C.c_int32), ("num_queries", C.c_int32), ("n_input_proj", C.c_int32),
        ("t_dim", C.c_int32), ("v_dim", C.c_int32), ("has_adapter", C.c_int32), ("v_motion_dim", C.c_int32),
        ("vid_proj_ln", LNorm * MAX_PROJ), ("vid_proj", Linear * MAX_PROJ),
        ("txt_proj_ln", LNorm * MAX_PROJ), ("txt_proj", Linear * MAX_PROJ),
        ("enc", EncLayer * MAX_LAYERS), ("dec", DecLayer * MAX_LAYERS),
        ("dec_norm", LNorm), ("query_embed", C.c_void_p), ("class_embed", Linear),
        ("span_embed", Linear * 3), ("saliency_proj", Linear), ("adapter", Linear * 2),
        ("pos_dim_t", C.c_void_p),
        ("txt_pos_embed", C.c_void_p), ("txt_pos_rows", C.c_int32), ("txt_pos_ln", LNorm),      # ABI 5: --use_txt_pos (NULL: off)
        ("pre_norm", C.c_int32), ("enc_norm", LNorm),                                            # ABI 5: --pre_norm (0: post-norm)
        ("table_max_v_l", C.c_int32),                                                            # ABI 8: tables for <= this many clips (0: 255)
    ]


class Layer0(C.Structure):
    _fields_ = [("qkv_vid", C.c_void_p), ("qkv_txt", C.c_void_p), ("pos_qk", C.c_void_p), ("pos_rows", C.c_void_p),
                ("max_v_l", C.c_int32),
                ("txt_pos", C.c_void_p), ("txt_pos_qk", C.c_void_p), ("n_txt", C.c_int64)]   # ABI 7: --use_txt_pos rows


class Taps(C.Structure):
    _fields_ = [("memory", C.c_void_p), ("hs", C.c_void_p), ("aux_logits", C.c_void_p),
                ("aux_spans", C.c_void_p)]


# video sessions (additive in ABI 8): cone_model_dims, cone_session, cone_session_params
SESSION_BF16, SESSION_CERTIFIED, SESSION_MAX_QUERIES = 1, 2, 64


class ModelDims(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("hidden_dim", "num_queries", "enc_layers", "t_dim", "v_dim", "v_motion_dim", "txt_pos",
                                         "long_windows")]


class Session(C.Structure):
    _fields_ = [("model", C.c_void_p), ("ctx_l", C.c_int64), ("flags", C.c_int32), ("v_dim", C.c_int32),
                ("hidden_dim", C.c_int32), ("vid_norm", C.c_void_p), ("adapted", C.c_void_p), ("adapted_bf16", C.c_void_p),
                ("err", C.c_void_p), ("vproj", C.c_void_p), ("qkv_vid", C.c_void_p)]


class SessionParams(C.Structure):
    _fields_ = [("max_v_l", C.c_int32), ("max_q_l", C.c_int32), ("clip_length", C.c_float), ("nms_thd", C.c_double),
                ("max_before", C.c_int32), ("max_after", C.c_int32)]


# video libraries (additive in ABI 8): cone_library
class Library(C.Structure):
    _fields_ = [("model", C.c_void_p), ("capacity", C.c_int64), ("flags", C.c_int32), ("v_dim", C.c_int32),
                ("hidden_dim", C.c_int32), ("vid_norm", C.c_void_p), ("adapted", C.c_void_p), ("adapted_bf16", C.c_void_p),
                ("vproj", C.c_void_p), ("qkv_vid", C.c_void_p)]


# certified library budgets (additive in ABI 8): cone_library_shadow
class LibraryShadow(C.Structure):
    _fields_ = [("model", C.c_void_p), ("capacity", C.c_int64), ("v_dim", C.c_int32), ("rows_bf16", C.c_void_p), ("err", C.c_void_p)]


_SIGNATURES = {
    "cone_last_error": (C.c_char_p, []),
    "cone_abi_version": (C.c_int, []),
    "cone_model_create": (C.c_int, [C.POINTER(Weights), C.POINTER(C.c_void_p)]),
    "cone_model_destroy": (None, [C.c_void_p]),
    "cone_adapter_norm_workspace": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "cone_adapter_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "cone_l2_normalize_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "cone_num_windows": (C.c_int64, [C.c_int64, C.c_int]),
    "cone_prefilter_scores_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "cone_prefilter_scores": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_prefilter_scores_split_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "cone_prefilter_scores_split": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_prefilter_batched": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # the opt-in bf16 pre-filter (additive in ABI 8)
    "cone_rows_to_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_adapter_norm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "cone_prefilter_scores_bf16_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "cone_prefilter_scores_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_prefilter_batched_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # the certified pre-filter (additive in ABI 8): bf16 scan, fp32 rescore, exact top-k windows
    "cone_prefilter_index_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_prefilter_topk_certified_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "cone_prefilter_topk_certified": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p] + [C.c_int] * 5
                                      + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "cone_topk_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_topk_windows_workspace": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "cone_topk_windows_ws": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "cone_project_workspace": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int64]),
    "cone_project_tokens": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "cone_mask_lengths": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_forward_workspace": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cone_forward_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Taps),
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_forward_packed_workspace": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Layer0)]),
    "cone_forward_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(Taps), C.POINTER(Layer0), C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_pos_table_rows": (C.c_int64, [C.c_int]),
    "cone_pos_tables": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_layer0_project_workspace": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "cone_layer0_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_layer0_text_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_clip_matching_workspace": (C.c_size_t, [C.c_void_p, C.c_int]),
    "cone_clip_matching_gathered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_clip_matching": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_window_table": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3
                          + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p]),
    "cone_compose_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_fuse_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_fuse_nms_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_temporal_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "cone_matcher_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_criterion_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "cone_adapter_nce": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "cone_prof_enable": (C.c_int, [C.c_int]),
    "cone_prof_collect": (C.c_int64, [C.c_void_p, C.c_int64]),
    "cone_eval_recall": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cone_eval_window_recall": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "cone_model_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    # video sessions (additive in ABI 8): the video half once, the query half as one call
    "cone_model_get_dims": (C.c_int, [C.c_void_p, C.POINTER(ModelDims)]),
    "cone_session_arena_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int]),
    "cone_session_workspace": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int]),
    "cone_session_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.POINTER(Session), C.c_void_p]),
    # cone_session_query_layout(tok_len (host), nq, max_q_l, ctx_l, K, Nq, max_v_l, <8 int32 outputs>, stream)
    "cone_session_query_layout": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int]
                                  + [C.c_void_p] * 8 + [C.c_void_p]),
    "cone_session_localize_workspace": (C.c_size_t, [C.c_void_p, C.POINTER(Session), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                                     C.c_int, C.POINTER(SessionParams)]),
    # cone_session_localize(m, session, tok, tok_len (host), nq, cls, K, n_cand, params, kept, n_kept, certified, ws, ws_bytes, stream)
    "cone_session_localize": (C.c_int, [C.c_void_p, C.POINTER(Session), C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                        C.c_int, C.c_int, C.POINTER(SessionParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    # video libraries (additive in ABI 8): many videos in one arena, one call for (video, query) pairs on any mix of them
    "cone_library_arena_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int]),
    "cone_library_open": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(Library)]),
    "cone_library_add_workspace": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "cone_library_add": (C.c_int, [C.c_void_p, C.POINTER(Library), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    # cone_library_query_layout(tok_len, q_row0, q_ctx_l (host), nq, max_q_l, K, Nq, max_v_l, <8 int32 outputs>, stream)
    "cone_library_query_layout": (C.c_int, [C.POINTER(C.c_int32)] * 3 + [C.c_int] * 5 + [C.c_void_p] * 8 + [C.c_void_p]),
    "cone_library_localize_workspace": (C.c_size_t, [C.c_void_p, C.POINTER(Library)] + [C.POINTER(C.c_int32)] * 3
                                        + [C.c_int, C.c_int, C.POINTER(SessionParams)]),
    # cone_library_localize(m, lib, q_row0, q_ctx_l (host), tok, tok_len (host), nq, cls, K, params, kept, n_kept, ws, ws_bytes, stream)
    "cone_library_localize": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                        C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.POINTER(SessionParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # library search (additive in ABI 8): stage A over many videos in one pass, the query half on the scanned lists
    "cone_library_scan_workspace": (C.c_size_t, [C.POINTER(Library), C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]),
    # cone_library_scan(m, lib, v_row0, v_ctx_l, v_hb_off (device), n_videos, total_hb, cls, nq, K, n_rank, params, widx, wval,
    # rank_slot, rank_val, ws, ws_bytes, stream)
    "cone_library_scan": (C.c_int, [C.c_void_p, C.POINTER(Library)] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.POINTER(SessionParams)] + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t,
                                                                                                    C.c_void_p]),
    "cone_library_localize_ranked_workspace": (C.c_size_t, [C.c_void_p, C.POINTER(Library)] + [C.POINTER(C.c_int32)] * 3
                                               + [C.c_int, C.c_int, C.POINTER(SessionParams)]),
    # cone_library_localize_ranked(<cone_library_localize's up to params>, pair_query, pair_slot (host), scan_widx, scan_wval
    # (device), scan_nq, scan_n_videos, scan_K, kept, n_kept, ws, ws_bytes, stream)
    "cone_library_localize_ranked": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                               C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.POINTER(SessionParams),
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # library maintenance (additive in ABI 8): moving resident rows bit for bit (compaction in place, resizing)
    "cone_library_move_stage_bytes": (C.c_size_t, [C.POINTER(Library), C.c_int64]),
    # cone_library_move_rows(m, src, dst, mv_src, mv_dst, mv_off (device), n_moves, total_rows, row_begin, row_end, stage,
    # stage_bytes, stream)
    "cone_library_move_rows": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(Library)] + [C.c_void_p] * 3 + [C.c_int64] * 4
                               + [C.c_void_p, C.c_size_t, C.c_void_p]),
    # library window budgets (additive in ABI 8): the W best windows of a query over a scan's lists, a window count per pair
    "cone_library_budget_workspace": (C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_int]),
    # cone_library_budget(wval (device), nq, n_videos, scan_K, W, n_pairs, pair_slot, pair_k, pair_best (device), ws, ws_bytes, stream)
    "cone_library_budget": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 4
                            + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "cone_library_localize_ragged_workspace": (C.c_size_t, [C.c_void_p, C.POINTER(Library)] + [C.POINTER(C.c_int32)] * 3
                                               + [C.c_int, C.POINTER(C.c_int32), C.POINTER(SessionParams), C.c_int]),
    # cone_library_localize_ragged(<cone_library_localize_ranked's, with pair_k (host) in place of K>): pair_query .. scan_wval all
    # NULL = the call's own stage A
    "cone_library_localize_ragged": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                               C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.POINTER(C.c_int32),
                                               C.POINTER(SessionParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]),
    # library moment search (additive in ABI 8): stage C over one candidate pool per query, the ragged call up to its candidates
    # cone_corpus_fuse_nms(cand, seg_off, seg_cand, seg_n, seg_tag (device), nq, n_seg, nms_thd, max_before, max_after, out_rows,
    # out_seg, out_n (device), stream)
    "cone_corpus_fuse_nms": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "cone_library_localize_candidates_workspace": (C.c_size_t, [C.c_void_p, C.POINTER(Library)] + [C.POINTER(C.c_int32)] * 3
                                                   + [C.c_int, C.POINTER(C.c_int32), C.POINTER(SessionParams), C.c_int]),
    # cone_library_localize_candidates(<cone_library_localize_ragged's, with cand (device) in place of kept, n_kept>)
    "cone_library_localize_candidates": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                   C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.POINTER(C.c_int32),
                                                   C.POINTER(SessionParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                   C.c_void_p]),
    # standing queries (additive in ABI 8): the plan of a poll over the cache of (query, window) candidate rows, and the scatter
    # cone_watch_plan(widx, wval (device), nq, K, stamp (device), n_win, ctx_l, W, Nq, miss_widx, miss_wval, n_miss, seg_off,
    # seg_cand, seg_n, seg_tag (device), stream)
    "cone_watch_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 8),
    # cone_watch_store(cand, miss_widx, n_miss (device), nq, K, n_win, ctx_l, Nq, cache, stamp (device), stream)
    "cone_watch_store": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 3),
    # standing queries over a library (additive in ABI 8): the plan over the budget's pairs and a cache of one slab per video
    # cone_watch_pool_plan(widx, wval, n_pairs, pair_slot, pair_k, v_ctx_l, v_win0, v_cap, stamp (device), nq, V, K, Wb, n_win_total,
    # W, Nq, miss_widx, miss_wval, pair_miss, seg_off, seg_cand, seg_n, seg_tag (device), stream)
    "cone_watch_pool_plan": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 7 + [C.c_void_p] * 8),
    # cone_watch_pool_store(cand, jobs (device), n_jobs, miss_widx, v_ctx_l, v_win0, v_cap (device), nq, V, K, n_win_total, Nq,
    # cache, stamp (device), stream)
    "cone_watch_pool_store": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 3),
    # certified library budgets (additive in ABI 8): a bf16 shadow of the adapted rows, the scan's lists for a budget from it
    "cone_library_shadow_bytes": (C.c_size_t, [C.POINTER(Library)]),
    "cone_library_shadow_open": (C.c_int, [C.POINTER(Library), C.c_void_p, C.c_size_t, C.POINTER(LibraryShadow)]),
    # cone_library_shadow_index(m, lib, shadow, row0, n_rows, stream)
    "cone_library_shadow_index": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(LibraryShadow), C.c_int64, C.c_int64, C.c_void_p]),
    # cone_library_scan_certified_workspace(lib, n_videos, total_hb, total_win, nq, K, W, n_cand)
    "cone_library_scan_certified_workspace": (C.c_size_t, [C.POINTER(Library), C.c_int64, C.c_int64, C.c_int64] + [C.c_int] * 4),
    # cone_library_scan_certified(m, lib, shadow, v_row0, v_ctx_l, v_hb_off, v_win_off (device), n_videos, total_hb, total_win, cls,
    # nq, K, W, n_cand, params, widx, wval, certified (device), ws, ws_bytes, stream)
    "cone_library_scan_certified": (C.c_int, [C.c_void_p, C.POINTER(Library), C.POINTER(LibraryShadow)] + [C.c_void_p] * 4
                                    + [C.c_int64] * 3 + [C.c_void_p] + [C.c_int] * 4 + [C.POINTER(SessionParams)] + [C.c_void_p] * 3
                                    + [C.c_void_p, C.c_size_t, C.c_void_p]),
    # cone_test_gemm(A, A2, a2_mod, W, bias, R, ln_g, ln_b, C, C2, ADD, M, N, K, flags, stream)
    "cone_test_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_void_p]),
    # cone_test_gemm_tall(<cone_test_gemm's up to flags>, lda, ldc, M_dev, n_cu, stream): the row GEMM's tall form
    "cone_test_gemm_tall": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    # the packed fp32 weight streams (tail_pack.hip) and the two weight-ring kernels on them
    "cone_test_f32_pack_tail_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    # cone_test_f32_pack_tail(Wo | None, W1, W2, ff, Wq | None, n_qkv, img, stream)
    "cone_test_f32_pack_tail": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_test_f32_pack_rows_bytes": (C.c_size_t, [C.c_int]),
    "cone_test_f32_packed_launches": (C.c_long, [C.c_int]),
    "cone_test_f32_pack_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # cone_test_gemm_tall_packed(A, W, bias, R, C, M, N, flags, M_dev, n_cu, img | None, stream)
    "cone_test_gemm_tall_packed": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # cone_test_tail_packed(A | None, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff, pre, OUT2, Wq, qb, QKV, n_qkv,
    #                       nw, n_cu, img | None, stream)
    "cone_test_tail_packed": (C.c_int, [C.c_void_p] * 13 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 3
                              + [C.c_void_p, C.c_void_p]),
    # cone_test_gemm_bf16(<cone_test_gemm's up to flags>, img, ldc, r_mod, M_dev, stream): the row GEMM of option general_bf16
    "cone_test_gemm_bf16_image_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "cone_test_gemm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_test_ffn": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p]),
    "cone_test_proj_ffn": (C.c_int, [C.c_void_p] * 13 + [C.c_int, C.c_int, C.c_void_p]),
    "cone_test_tail_form": (C.c_int, [C.c_void_p] * 13 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                                               C.c_void_p, C.c_void_p]),
    "cone_test_proj_ffn_spread_scratch_bytes": (C.c_size_t, [C.c_int]),
    "cone_test_proj_ffn_spread": (C.c_int, [C.c_void_p] * 13 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_test_ffn_split_image_bytes": (C.c_size_t, [C.c_int]),
    "cone_test_ffn_split": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cone_test_rows_split_image_bytes": (C.c_size_t, [C.c_int]),
    "cone_test_rows_split": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cone_test_proj_split_image_bytes": (C.c_size_t, []),
    "cone_test_proj_ffn_split": (C.c_int, [C.c_void_p] * 13 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    # cone_test_tail_mc(A | None, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff, r_idx, R2, M_dev, pre, OUT2, Wq, qb, QKV,
    #                   n_qkv, lda, ldr, ldo, ldo2, ldq, n_cu, img, wo_img, q_img, pack, stream)
    "cone_test_tail_mc": (C.c_int, [C.c_void_p] * 13 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
                          + [C.c_int] * 7 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]),
    # cone_test_rows_mc(X, W, bias, C, M, N, img, pack, ldx, ldc, M_dev, n_cu, stream)
    "cone_test_rows_mc": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int,
                                                                                                        C.c_void_p]),
    "cone_test_enc_attn": (C.c_int, [C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cone_test_dec_cross": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "cone_test_dec_cross_slab_floats": (C.c_size_t, []),
    # cone_test_enc_attn_txt(mode, QKV, qkv_vid, qkv_txt, pos_qk, txt_pos_qk, vrow0, vlen, trow0, off, OUT, B, Lmax, zero_row, stream)
    "cone_test_enc_attn_txt": (C.c_int, [C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # cone_test_small_attn(Q, ldq, K, ldk, V, ldv, OUT, ldo, off, B, nq, Lmax, stream)
    "cone_test_small_attn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # cone_test_dec_cross_ex(DQ, XP, X, pos_rows, vlen, off, Wk, WvT, bv, OUT, B, nq, Lmax, variant, qk_slabs, sal_w, sal_b, sal,
    # sal_ld, stream)
    "cone_test_dec_cross_ex": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "cone_test_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                      C.c_void_p]),
    # cone_test_gen_attn(Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, B, nq, heads, head_dim, kcap, stream)
    "cone_test_gen_attn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    # the glue kernels of stage B, one entry per launcher (include/cone_hip.h: the operand lists)
    "cone_test_grid_limit_y": (C.c_int, []),
    "cone_test_scan_lengths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cone_test_compact_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_int, C.c_void_p]),
    "cone_test_pack_pos": (C.c_int, [C.c_void_p] * 11 + [C.c_int, C.c_int] + [C.c_void_p] * 4),
    "cone_test_gen_pack_pos": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 3 + [C.c_void_p] * 4),
    "cone_test_pack_l0": (C.c_int, [C.c_void_p] * 15 + [C.c_int, C.c_int, C.c_void_p]),
    "cone_test_row_index": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]),
    "cone_test_add_pos_rows": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 3),
    "cone_test_txt_pos_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3),
    "cone_test_gen_txt_pos_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int,
                                                                                                    C.c_void_p, C.c_void_p]),
    "cone_test_saliency": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cone_test_gen_saliency": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cone_test_rowdot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                                   C.c_void_p]),
    "cone_test_gen_rowdot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p]),
    "cone_test_tile_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "cone_test_tile_rows2": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int64, C.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


class ConeHipError(RuntimeError):
    pass


def load():
    """Load libcone_hip.so; raises if it has not been built (python -m cone_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ConeHipError(
            f"{LIB_PATH} is missing: build the HIP extension with `python -m cone_amd.build` "
            "(hipcc, gfx950). cone_amd has no CPU fallback.")
    # torch ships its own libamdhip64.so.7; importing torch first makes our DT_NEEDED resolve to that
    # copy, so the process has ONE HIP runtime and torch's streams / allocations are ours too.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.cone_abi_version() != 8:
        raise ConeHipError("libcone_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


_pylists = None


def pylists():
    """The host-side list builder (cone_amd/csrc/pylists.c, ctypes.PyDLL: the call keeps the GIL)."""
    global _pylists
    if _pylists is None:
        path = os.path.join(HERE, "_cone_pylists.so")
        if not os.path.exists(path):
            raise ConeHipError(f"{path} is missing: build with `python -m cone_amd.build`")
        lib = C.PyDLL(path)
        fn = lib.cone_fill_predicted_times
        fn.restype = C.py_object
        fn.argtypes = [C.py_object, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.py_object]
        _pylists = lib
    return _pylists


def check(rc: int):
    if rc != 0:
        raise ConeHipError(f"libcone_hip error {rc}: {load().cone_last_error().decode()}")


def sized(nbytes: int) -> int:
    """The result of a ``*_workspace`` / ``*_bytes`` entry: a size of 0 means the call was refused."""
    if nbytes == 0:
        raise ConeHipError(f"libcone_hip error: {load().cone_last_error().decode()}")
    return nbytes


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    import torch
    if t is None:
        return None
    if not t.is_cuda:
        raise ConeHipError("expected a tensor on the GPU")
    if not t.is_contiguous():
        raise ConeHipError("expected a contiguous tensor")
    if dtype is not None and t.dtype != dtype:
        raise ConeHipError(f"expected dtype {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def stream():
    """The current HIP stream of the current device as a void*.  (The raw-stream getter is what torch's own compiled
    code paths call; it skips the Stream object that torch.cuda.current_stream() builds on every call -- the front of a
    step is ~30 launches issued while the GPU waits for the host.)"""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return C.c_void_p(raw(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
