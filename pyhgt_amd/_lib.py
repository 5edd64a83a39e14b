"""ctypes binding of libhgt_hip.so (the C ABI declared in include/hgt_hip.h).

The library is built in-tree (pyhgt_amd/lib/libhgt_hip.so, see __graft_entry__.build() or
`make -C pyhgt_amd/csrc`).  There is NO fallback: if the shared object is missing or a call
returns an error code, a RuntimeError is raised.
"""
import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HGT_LIB_PATH", os.path.join(_HERE, "lib", "libhgt_hip.so"))   # override: development A/B builds

HGT_RTE_LEN = 240
HGT_N_PHASE_EVENTS = 7
HGT_FLAG_NO_FUSED_UPDATE = 1
HGT_FLAG_VALU_AGGREGATE = 2
HGT_FLAG_MFMA_LOGITS = 4
HGT_FLAG_VALU_LOGITS = 8
HGT_FLAG_ITEM_AGGREGATE = 16
HGT_FLAG_NO_ITEM_AGGREGATE = 32
HGT_FLAG_FUSED_ANY_SIZE = 64
HGT_FLAG_DETERMINISTIC_HUBS = 128
# (bits 256 and 512 are retired -- include/hgt_hip.h)
HGT_FLAG_XS_GEMM_ALWAYS = 1024
HGT_FLAG_XS_GEMM_NEVER = 2048
HGT_FLAG_NO_TILE_GEMM = 4096
HGT_FLAG_NO_MERGE_UPDATE = 8192
HGT_FLAG_NO_COOP_EDGE = 16384
HGT_FLAG_COOP_EDGE_ALWAYS = 32768
HGT_FLAG_KSIDE_LOGITS = 65536
HGT_FLAG_NO_KSIDE_LOGITS = 131072
HGT_FLAG_KSIDE_LANE_GATHER = 262144
HGT_LINEAR_FORCE_XS = 0x100
HGT_LINEAR_NO_XS = 0x200
HGT_LINEAR_NO_TILE = 0x400
HGT_LINEAR_TANH = 0x1000
HGT_FEATURE_DETERMINISTIC_TRAINING = 2
HGT_STACK_MAX_PIECES = 256
HGT_SAMPLER_MAX_TYPES = 16
HGT_SAMPLER_MAX_TRIPLES = 48
HGT_SAMPLER_MAX_NUMBER = 1024
HGT_SAMPLER_HUB_DEG = 512
HGT_SAMPLER_TIME_NONE = -2 ** 31
HGT_SAMPLER_MAX_BATCH = 64
HGT_TRIM_MAX_LAYERS = 8
HGT_VIEW_TILE = 512          # entries of the whole-graph view's entry space one wavefront takes (a workgroup takes four such tiles)
HGT_VIEW_BAD_TIME = 1
HGT_NB_CHUNK = 1024          # entries of a row one wavefront of the neighbourhood walk takes; a longer row is split into chunks
HGT_NB_WAVE_ROWS = 64        # rows of a level whose totals one wavefront of the numbering kernel sums (the wavefront width)
HGT_NB_BAD_SEED, HGT_NB_BAD_TIME = 1, 2
HGT_NB_HEAD_N, HGT_NB_HEAD_DEG, HGT_NB_HEAD_CHUNKS, HGT_NB_HEAD_KEPT, HGT_NB_HEAD_FLAGS = 0, 1, 2, 3, 4
HGT_NB_HEAD_TYPE_BEGIN, HGT_NB_HEAD_TYPE_END, HGT_NB_HEAD_WORDS = 8, 24, 40


class HgtLayout(C.Structure):
    _fields_ = [("d_k", C.c_int32), ("dk_pad", C.c_int32), ("d_pad", C.c_int32), ("vec", C.c_int32), ("heads", C.c_int32)]


class HgtPlanSizes(C.Structure):
    _fields_ = [("plan_bytes", C.c_uint64), ("tmp_bytes", C.c_uint64), ("max_items", C.c_int64), ("n_bins", C.c_int64)]


class HgtPlanRows(C.Structure):
    _fields_ = [("rows_all", C.c_void_p), ("off_all", C.c_void_p), ("rows_q", C.c_void_p), ("off_q", C.c_void_p)]


class HgtConvArgs(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64), ("n_edges", C.c_int64),
        ("in_dim", C.c_int32), ("out_dim", C.c_int32), ("n_types", C.c_int32), ("n_relations", C.c_int32),
        ("n_heads", C.c_int32),
        ("use_norm", C.c_int32), ("use_rte", C.c_int32), ("precision", C.c_int32), ("want_att", C.c_int32),
        ("n_q_rows", C.c_int64),
        ("x", C.c_void_p), ("node_type", C.c_void_p), ("plan", C.c_void_p),
        ("w_qkv", C.c_void_p), ("b_qkv", C.c_void_p), ("w_a", C.c_void_p), ("b_a", C.c_void_p),
        ("relation_att", C.c_void_p), ("relation_msg", C.c_void_p), ("relation_pri", C.c_void_p),
        ("skip", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p),
        ("rte_emb", C.c_void_p), ("rte_w", C.c_void_p), ("rte_b", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64),
        ("out", C.c_void_p), ("att_out", C.c_void_p),
        ("phase_events", C.c_void_p),
        ("update_mode", C.c_int32),
        ("mid_w", C.c_void_p), ("mid_b", C.c_void_p), ("out_w", C.c_void_p), ("out_b", C.c_void_p),
        ("out_ln_w", C.c_void_p), ("out_ln_b", C.c_void_p),
        ("stage", C.c_int32), ("proj_rows", C.c_void_p), ("proj_off", C.c_void_p), ("proj_n", C.c_int64),
        ("prepared", C.c_void_p), ("prepared_bytes", C.c_uint64), ("prepared_valid", C.c_int32),
        ("plan_no_hubs", C.c_int32),
        ("flags", C.c_int32),
        ("slice_index", C.c_int32),
        ("slice_count", C.c_int32),
        ("q_begin", C.c_int64), ("q_end", C.c_int64),
        ("item_begin", C.c_int32), ("item_end", C.c_int32),
        ("proj_c24", C.c_void_p), ("proj_c24_row0", C.c_int64),
    ]


class HgtSamplerType(C.Structure):
    _fields_ = [("score", C.c_void_p), ("stamp", C.c_void_p), ("serial", C.c_void_p), ("sampled", C.c_void_p), ("cand", C.c_void_p),
                ("counts", C.c_void_p), ("n_nodes", C.c_int32), ("cap_sampled", C.c_int32), ("cap_cand", C.c_int32), ("reserved", C.c_int32)]


class HgtSamplerTriple(C.Structure):
    _fields_ = [("indptr", C.c_void_p), ("src", C.c_void_p), ("time", C.c_void_p), ("tgt_type", C.c_int32), ("src_type", C.c_int32),
                ("rel_id", C.c_int32), ("reserved", C.c_int32)]


class HgtSamplerMask(C.Structure):
    _fields_ = [("tgt_below", C.c_int32), ("src_below", C.c_int32)]


class HgtGraphCsr(C.Structure):
    _fields_ = [("indptr", C.c_void_p), ("nbr", C.c_void_p)]


class HgtViewTriple(C.Structure):
    _fields_ = [("indptr", C.c_void_p), ("src", C.c_void_p), ("time", C.c_void_p), ("tgt_flags", C.c_void_p), ("src_flags", C.c_void_p),
                ("tgt_time", C.c_void_p), ("src_time", C.c_void_p), ("first", C.c_int64), ("n_rows", C.c_int32), ("tgt_off", C.c_int32),
                ("src_off", C.c_int32), ("rel_id", C.c_int32)]


class HgtNbType(C.Structure):
    _fields_ = [("mark", C.c_void_p), ("feat", C.c_void_p), ("ld", C.c_int64), ("row_off", C.c_int64), ("n_nodes", C.c_int32),
                ("reserved", C.c_int32)]


class HgtNbTriple(C.Structure):
    _fields_ = [("indptr", C.c_void_p), ("src", C.c_void_p), ("time", C.c_void_p), ("tgt_flags", C.c_void_p), ("src_flags", C.c_void_p),
                ("tgt_time", C.c_void_p), ("src_time", C.c_void_p), ("tgt_type", C.c_int32), ("src_type", C.c_int32),
                ("rel_id", C.c_int32), ("reserved", C.c_int32)]


GRAPH_MEAN_CHUNK = 256      # HGT_GRAPH_MEAN_CHUNK: the most terms of a row one wavefront of hgt_neighbour_mean adds
HGT_GRAPH_TIME_BY_ROW = 0
HGT_GRAPH_TIME_BY_NBR = 1
RANK_LIST_CAP = 1024    # HGT_RANK_LIST_CAP: positives a pass of hgt_rank_metrics holds
CLASS_LOSS_WAVE_COLS = 256   # HGT_CLASS_LOSS_WAVE_COLS: the longest row of hgt_class_loss that takes a wavefront
OPTIM_CHUNK = 4096          # HGT_OPTIM_CHUNK: the most elements of one tensor a workgroup of the optimizer kernels takes
TOPK_MAX_K = 128           # HGT_TOPK_MAX_K: the most candidates per query hgt_matcher_topk returns
PREDICT_MAX_SPLITS = 8     # HGT_PREDICT_MAX_SPLITS: the most splits hgt_class_predict counts in one call
ABI_VERSION = 8          # HGT_ABI_VERSION of include/hgt_hip.h this binding was written against

_i32, _i64, _u64, _vp = C.c_int32, C.c_int64, C.c_uint64, C.c_void_p

# name -> (restype, argtypes); every symbol include/hgt_hip.h declares
SIGNATURES = {
    "hgt_strerror": (C.c_char_p, [C.c_int]),
    "hgt_abi_version": (C.c_int, []),
    "hgt_build_features": (C.c_int, []),
    "hgt_layout_for": (C.c_int, [_i32, _i32, C.POINTER(HgtLayout)]),
    "hgt_plan_sizes_for": (C.c_int, [_i64, _i64, _i32, _i32, C.POINTER(HgtPlanSizes)]),
    "hgt_plan_constants": (C.c_int, [C.POINTER(_i32), C.POINTER(_i32)]),
    "hgt_plan_item_edges": (C.c_int, [_i64, C.POINTER(_i32)]),
    "hgt_plan_row_lists": (C.c_int, [_vp, _i64, _i64, _i32, _i32, C.POINTER(HgtPlanRows)]),
    "hgt_plan_tile_items_offset": (C.c_int, [_i64, _i64, _i32, _i32, C.POINTER(_u64), C.POINTER(_i64)]),
    "hgt_plan_build": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _u64, _vp, _u64, _vp]),
    "hgt_plan_from_sorted": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _u64, _vp, _u64, _vp]),
    "hgt_typed_linear": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                   _i32, _i32, _i32, _i32, _vp]),
    "hgt_split_weights_bytes": (C.c_int, [_i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_split_weights": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "hgt_typed_linear_bf16x3": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                          _i32, _i32, _i32, _vp]),
    "hgt_linear_update_bf16x3": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                           _i32, _vp, _vp]),
    "hgt_split_weights_f16": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "hgt_typed_linear_xs_schedule": (C.c_int, [_vp, _i32, _i64, _i32, _i32, _vp, _i64, C.POINTER(_i64)]),
    "hgt_typed_linear_f16x3": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                         _i32, _i32, _i32, _vp]),
    "hgt_linear_update_f16x3": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                          _i32, _vp, _vp]),
    "hgt_zero_rows": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "hgt_relation_pack": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "hgt_edge_logits": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hgt_edge_logits_mfma": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "hgt_relation_kside_bytes": (C.c_int, [_i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_relation_kside_pack": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "hgt_edge_logits_kside": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "hgt_kside_image_map": (C.c_int, [_i32, _vp, _vp, _vp]),
    "hgt_kside_gather_map": (C.c_int, [_vp, _vp]),
    "hgt_edge_logits_range": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "hgt_edge_aggregate_update_range": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _i64, _i32, _i32]),
    "hgt_hub_workspace_bytes_ex": (C.c_int, [_i64, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_edge_aggregate_ex": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp, _i32, _vp]),
    "hgt_edge_logits_slice": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "hgt_edge_aggregate_slice": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp,
                                           _i32, _i32, _vp, _i32, _i32, _vp]),
    "hgt_edge_aggregate_slice_ex": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp,
                                              _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "hgt_edge_softmax": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp]),
    "hgt_edge_aggregate": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "hgt_edge_aggregate_f16x3": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "hgt_relation_frag_pack_f16": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "hgt_edge_aggregate_items_bytes": (C.c_int, [_i64, _i32, _i32, C.POINTER(_u64)]),
    "hgt_edge_spmm_items": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _u64, _vp]),
    "hgt_edge_aggregate_items_update": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _u64, _vp, _vp, _i32,
                                                  _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "hgt_edge_aggregate_items": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp, _u64, _vp]),
    "hgt_plan_header_to_host": (C.c_int, [_vp, _vp, _vp]),
    "hgt_relation_frag_bytes": (C.c_int, [_i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_relation_frag_pack": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "hgt_hub_workspace_bytes": (C.c_int, [_i64, _i32, _i32, C.POINTER(_u64)]),
    "hgt_att_export": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "hgt_edge_aggregate_update": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "hgt_edge_aggregate_update_f16x3": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "hgt_edge_spmm": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "hgt_edge_softmax_bwd": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "hgt_edge_gather_sorted": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "hgt_head_dot": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "hgt_relation_outer": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hgt_relation_outer_wide": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hgt_node_update_bwd_ex": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                         _vp]),
    "hgt_single_group_offsets": (C.c_int, [_vp, _i32, _vp, _vp]),
    "hgt_node_update_bwd": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hgt_gelu_bwd": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "hgt_mul_inplace": (C.c_int, [_vp, _vp, _i64, _vp]),
    "hgt_typed_wgrad": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i64, _vp]),
    "hgt_typed_wgrad_bf16x3": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
    "hgt_typed_colsum": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _vp, _i64, _vp]),
    # the atomic-free forms of the backward (deterministic=True): the atomic form's arguments + (workspace, bytes) in front of the stream
    "hgt_node_update_bwd_det_bytes": (C.c_int, [_i64, _i32, _i32, C.POINTER(_u64)]),
    "hgt_node_update_bwd_det": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                          _vp, _u64, _vp]),
    "hgt_typed_wgrad_det_bytes": (C.c_int, [_i32, _i64, _i32, _i32, C.POINTER(_u64)]),
    "hgt_typed_wgrad_det": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i64, _vp, _u64, _vp]),
    "hgt_typed_wgrad_bf16x3_det_bytes": (C.c_int, [_i32, _i64, _i32, _i32, C.POINTER(_u64)]),
    "hgt_typed_wgrad_bf16x3_det": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _u64, _vp]),
    "hgt_typed_colsum_det_bytes": (C.c_int, [_i32, _i64, _i32, C.POINTER(_u64)]),
    "hgt_typed_colsum_det": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _vp, _i64, _vp, _u64, _vp]),
    "hgt_relation_outer_det_bytes": (C.c_int, [_i64, _i64, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_relation_outer_det": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "hgt_relation_outer_wide_det_bytes": (C.c_int, [_i64, _i64, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_relation_outer_wide_det": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "hgt_edge_spmm_det_bytes": (C.c_int, [_i64, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_edge_spmm_det": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _u64, _vp]),
    "hgt_log_softmax_rows": (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "hgt_row_dot": (C.c_int, [_vp, _vp, _i64, _i32, C.c_float, _vp, _vp]),
    "hgt_node_update": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp]),
    "hgt_node_update_ex": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _i32, _vp, _vp]),
    "hgt_tanh_inplace": (C.c_int, [_vp, _i64, _vp]),
    "hgt_gather_rows_c24": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp]),
    "hgt_unpack_rows_c24": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _vp]),
    "hgt_gather_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp]),
    "hgt_scatter_add_rows": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "hgt_conv_workspace_bytes": (C.c_int, [_i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_conv_workspace_bytes_ex": (C.c_int, [_i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_conv_prepared_bytes": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_conv_forward": (C.c_int, [C.POINTER(HgtConvArgs), _vp]),
    # counter-based dropout (csrc/hgt_dropout.hip): (array, n, seed, offset, keep, stream)
    "hgt_dropout_mask": (C.c_int, [_vp, _i64, _u64, _u64, C.c_float, _vp]),
    "hgt_dropout_apply": (C.c_int, [_vp, _i64, _u64, _u64, C.c_float, _vp]),
    # stacking sampled batches (csrc/hgt_stack.hip): (src, dst, time, rel_ptr[B][R+1], type_off[B][T+1], edge_off_host, node_off_host,
    # B, T, R, src_out, dst_out, time_out, rel_ptr_out, type_off_out, node_map, edge_map, tmp, tmp_bytes, stream)
    "hgt_stack_tmp_bytes": (C.c_int, [_i32, _i32, _i32, C.POINTER(_u64)]),
    "hgt_stack_sorted": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _u64, _vp]),
    # device sampler (csrc/hgt_sampler.hip): every call starts with (types_host, n_types[, triples_host, n_triples])
    "hgt_sampler_seed": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp]),
    "hgt_sampler_add_budget": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _vp, _i64, _vp]),
    "hgt_sampler_select": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _u64, _vp, _vp, _i64, _vp]),
    "hgt_sampler_induce_slots": (C.c_int, [_vp, _i32, _vp, _i32, C.POINTER(_i64)]),
    "hgt_sampler_induce_count": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hgt_sampler_induce_fill": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hgt_sampler_reset": (C.c_int, [_vp, _i32, _vp]),
    # task batches: the induce calls with (masks_host) in front of the stream; labels (csrc/hgt_sampler_labels.hip): (triple_host,
    # n_tgt_nodes, n_src_nodes, ids, n, col_of, n_cols, has_window, t_min, t_max, dist_out, ld, index_out, count_out, stream)
    "hgt_sampler_induce_count_masked": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hgt_sampler_induce_fill_masked": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                 _vp]),
    "hgt_sampler_labels": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    # batched device sampler: the single calls with n_batch behind the tables, a host array of n_batch Philox seeds in place of the
    # seed, and in the fill calls (sizes, offs_out) behind type_off; gather_features: (features_host, type_nodes_host, n_types, n_batch,
    # width, type_off, offs, node_id, n_nodes, out, stream)
    "hgt_sampler_seed_batched": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp]),
    "hgt_sampler_add_budget_batched": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp]),
    "hgt_sampler_select_batched": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "hgt_sampler_induce_count_batched": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hgt_sampler_induce_count_masked_batched": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hgt_sampler_induce_fill_batched": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp,
                                                  _vp, _vp, _vp]),
    "hgt_sampler_induce_fill_masked_batched": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                                                         _vp, _vp, _vp, _vp, _vp]),
    "hgt_sampler_reset_batched": (C.c_int, [_vp, _i32, _i32, _vp]),
    "hgt_sampler_gather_features": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp]),
    # scoring task batches (csrc/hgt_task_metrics.hip): (scores, labels, index, row_ptr, n_rows, n_cols, ld_scores, ld_labels, k, ndcg_out,
    # rr_out, stream); the loss: (scores, row_ptr, n_seg, max_len, loss_out, lse_out, stream) and (scores, row_ptr, n_seg, max_len, lse,
    # grad_loss, grad_scores, stream)
    "hgt_rank_metrics": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i32, _vp, _vp, _vp]),
    "hgt_segment_first_nll": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "hgt_segment_first_nll_bwd": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    # classification losses (csrc/hgt_task_loss.hip): (logits, ld, n_rows, n_cols, labels, ld_labels, index, columns, width, count, loss_out,
    # lse_out, wsum_out, stream) and (..., count, lse, wsum, grad_loss, grad_logits, ld_grad, stream); the labels as column lists
    # (csrc/hgt_sampler_labels.hip): hgt_sampler_labels's arguments up to t_max, then (columns_out, width, count_out, stream)
    "hgt_class_loss": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "hgt_class_loss_bwd": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "hgt_sampler_label_columns": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    # voted evaluation (csrc/hgt_task_vote.hip): (scores, ld, n_rows, n_cols, ids, n_table, label, split, n_splits, pred_out, counts_out,
    # stream) and (logits, ld, n_cols, ids, piece_ptr_host, n_pieces, slot_of, n_nodes, votes, ld_votes, count, n_slots, stream)
    "hgt_class_predict": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp]),
    "hgt_vote_add": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _vp, _i32, _vp]),
    # the optimizer step (csrc/hgt_optim.hip): (numel_host, n_tensors, chunks_host, capacity, n_chunks_host); (n_tensors, n_groups,
    # n_chunks, step_bytes, groups_offset, chunk_bytes, partials_bytes); (tensors, n_tensors, groups, n_groups, chunks, n_chunks, partials,
    # stream); (partials, n_chunks, total_norm, stream); (tensors .. n_chunks, total_norm, max_norm, stream)
    "hgt_optim_constants": (C.c_int, [C.POINTER(_i32)]),
    "hgt_optim_chunk_table": (C.c_int, [_vp, _i32, _vp, _i64, C.POINTER(_i64)]),
    "hgt_optim_tables_bytes": (C.c_int, [_i32, _i32, _i64, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "hgt_grad_sqnorm": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i64, _vp, _vp]),
    "hgt_grad_norm_join": (C.c_int, [_vp, _i64, _vp, _vp]),
    "hgt_adamw_step": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i64, _vp, C.c_float, _vp]),
    # the resident graph from raw edge lists (csrc/hgt_graph_build.hip): (E, ws_bytes); (rows, row_stride, nbrs, nbr_stride, id_bytes,
    # edge_time, node_time, node_time_by, E, n_rows, n_nbrs, indptr, nbr_out, time_out, status, ws, ws_bytes, stream); (n_entries, d,
    # ws_bytes); (csrs_host, n_csr, x, ldx, n_rows, n_entries, d, out, ldo, ws, ws_bytes, stream)
    "hgt_graph_csr_bytes": (C.c_int, [_i64, C.POINTER(_u64)]),
    "hgt_graph_csr_build": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "hgt_neighbour_mean_bytes": (C.c_int, [_i64, _i32, C.POINTER(_u64)]),
    "hgt_neighbour_mean": (C.c_int, [_vp, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _u64, _vp]),
    # seed-trimmed graphs (csrc/hgt_trim.hip): (N, E, L, tmp_bytes); (edge_index, stride_row, stride_col, N, E, seeds, n_seeds, L, tmp,
    # tmp_bytes, stream); (edge_index, stride_row, stride_col, edge_type, edge_time, node_type, N, E, seeds, n_seeds, L, tmp, tmp_bytes,
    # hop, order, new_id, edge_order, node_type_out, edge_index_out, edge_type_out, edge_time_out, out_rows, counts, counts_host, stream)
    "hgt_trim_tmp_bytes": (C.c_int, [_i64, _i64, _i32, C.POINTER(_u64)]),
    "hgt_trim_hops": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _vp, _u64, _vp]),
    "hgt_trim_fill": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp]),
    # whole-graph view (csrc/hgt_graph_view.hip): (n_entries, tmp_bytes); (table_dev, n_triples, n_relations, n_entries, filtered,
    # has_max_time, max_time, has_time, src32, dst32, time32, edge_index, edge_index_stride, edge_type, edge_time, rel_ptr, tmp,
    # tmp_bytes, head_host_pinned, stream)
    "hgt_view_tmp_bytes": (C.c_int, [_i64, C.POINTER(_u64)]),
    "hgt_view_build": (C.c_int, [_vp, _i32, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    # exact neighbourhoods (csrc/hgt_neighbourhood.hip): every call starts with (types_dev, n_types); include/hgt_hip.h has the rest
    "hgt_nb_constants": (C.c_int, [C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "hgt_nb_sort_bytes": (C.c_int, [_i64, _i32, C.POINTER(_u64)]),
    "hgt_nb_seeds": (C.c_int, [_vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hgt_nb_number": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i64, _vp, _vp, _u64, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "hgt_nb_expand": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "hgt_nb_fill": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _vp,
                              _vp, _vp, _i64, _vp, _vp]),
    "hgt_nb_finish": (C.c_int, [_vp, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "hgt_nb_reset": (C.c_int, [_vp, _i32, _vp, _i64, _vp]),
    # matcher retrieval (csrc/hgt_matcher_topk.hip): (n_cand, n_query, k, chunk_rows, bytes); (tx, ld_x, n_cand, ty, ld_y, n_query, d, scale,
    # k, chunk_rows, values_out, indices_out, ws, ws_bytes, stream); (tx .. scale, chunk_rows, index, rank_out, ws, ws_bytes, stream)
    "hgt_matcher_topk_bytes": (C.c_int, [_i64, _i64, _i32, _i64, C.POINTER(_u64)]),
    "hgt_matcher_topk": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, C.c_float, _i32, _i64, _vp, _vp, _vp, _u64, _vp]),
    "hgt_matcher_rank": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, C.c_float, _i64, _vp, _vp, _vp, _u64, _vp]),
}

_lib = None


def load():
    """Load libhgt_hip.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                "pyhgt_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C pyhgt_amd/csrc`; there is no CPU/PyTorch fallback for HGTConv" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        if lib.hgt_abi_version() != ABI_VERSION:
            raise RuntimeError("pyhgt_amd: ABI version mismatch in %s" % LIB_PATH)
        _lib = lib
    return _lib


def check(code, what):
    if code != 0:
        msg = load().hgt_strerror(code).decode()
        raise RuntimeError("pyhgt_amd: %s failed: %s (code %d)" % (what, msg, code))


def layout_for(d_out, n_heads):
    lay = HgtLayout()
    check(load().hgt_layout_for(d_out, n_heads, C.byref(lay)), "hgt_layout_for(d=%d, heads=%d)" % (d_out, n_heads))
    return lay


def ptr(t):
    """the address of a tensor for a C call; None (NULL) for None or an empty tensor"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def table_to_device(table, dev):
    """a ctypes array of structures -> its bytes as a uint8 tensor on `dev`"""
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)


_pinned = threading.local()


def pinned(name, words, dtype):
    """The pinned host buffer `name` of this thread for a call's read-back, allocated on first use and kept: allocating pinned memory
    costs more than the calls it serves.  A buffer is busy from its copy to its read; the same call makes both, so a buffer per thread
    is never handed out while busy."""
    buf = getattr(_pinned, name, None)
    if buf is None:
        buf = torch.zeros(words, dtype=dtype).pin_memory()
        setattr(_pinned, name, buf)
    return buf
