"""ctypes binding of ``libtgm_amd.so`` (C ABI: ``include/tgm_amd.h``).

The library is built in-tree by ``__graft_entry__.build()`` /
``tgm_amd/csrc/Makefile``.  There is deliberately NO fallback: if the shared
object is missing, or no ROCm device is visible, every compute entry point
raises :class:`NativeLibraryError`.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_int32, c_int64, c_size_t, c_void_p
from typing import Optional

import torch

from .exceptions import NativeLibraryError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libtgm_amd.so')

# every symbol include/tgm_amd.h declares: name -> (restype, argtypes)
_P = c_void_p
SIGNATURES = {
    'tgmx_version': (c_int32, []),
    'tgmx_abi_sizeof': (c_size_t, [c_int32]),
    'tgmx_last_error': (c_char_p, []),
    'tgmx_event_create': (c_int32, [ctypes.POINTER(c_void_p)]),
    'tgmx_event_destroy': (c_int32, [_P]),
    'tgmx_event_elapsed_ms': (c_int32, [_P, _P, ctypes.POINTER(ctypes.c_float)]),
    'tgmx_recency_lookup_csr': (
        c_int32,
        [_P, _P, _P, c_int32, _P, _P, c_int64, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P],
    ),
    'tgmx_ring_lookup': (
        c_int32,
        [_P, _P, _P, c_int32, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P],
    ),
    'tgmx_ring_update': (
        c_int32,
        [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int64, c_int64, c_int32, c_int32, _P, _P, _P],
    ),
    'tgmx_ring_reset': (c_int32, [_P, _P, c_int32, c_int32, _P]),
    'tgmx_time2vec': (c_int32, [_P, c_int32, _P, _P, c_int32, c_int64, _P, _P]),
    'tgmx_gather_rows': (c_int32, [_P, c_int64, c_int32, _P, c_int64, _P, c_int64, _P]),
    'tgmx_tgat_rres': (c_int32, [_P, c_int64, c_int32, _P, _P, c_int32, c_int32, c_int64, _P, c_int64, _P]),
    'tgmx_sgemm_nt': (
        c_int32,
        [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, c_int32, c_int32, c_int64, c_int64, c_int64, _P],
    ),
    'tgmx_tgat_attn_reduce': (
        c_int32,
        [_P, _P, c_int32, _P, c_int32, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int64, ctypes.c_float, c_int32, _P, _P, _P, _P],
    ),
    'tgmx_tgn_store': (c_int32, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int64, c_int64, _P, _P, _P, _P, _P, _P]),
    'tgmx_tgn_aggregate': (
        c_int32,
        [_P, c_int64, _P, _P, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, c_int32, _P, _P, c_int32, c_int32, _P, _P, _P, c_int64, _P],
    ),
    'tgmx_tgn_commit_assoc': (c_int32, [_P, _P, c_int64, _P, c_int64, _P, _P, c_int32, c_int32, _P, _P, _P, _P]),
    'tgmx_tgn_store_batch': (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    'tgmx_tgn_edge_list': (c_int32, [_P, _P, _P, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, _P]),
    'tgmx_tgn_compact_workspace_bytes': (c_size_t, [c_int32]),
    'tgmx_tgn_compact': (c_int32, [_P, _P, _P, _P, c_int32, _P, _P, _P, c_int32, _P, _P, _P, _P, c_size_t, _P]),
    'tgmx_tgn_edge_list_by_id': (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, _P]),
    'tgmx_tgn_gru_gate': (c_int32, [_P, _P, _P, c_int32, c_int64, _P, _P]),
    'tgmx_tgn_commit': (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int64, _P, _P, _P]),
    'tgmx_tconv_edge_attr': (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int64, _P, _P]),
    'tgmx_tconv_attend': (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, ctypes.c_float, _P, _P, _P]),
    'tgmx_gcn_norm_dense': (c_int32, [_P, _P, _P, c_int64, c_int64, ctypes.c_float, c_int32, _P, c_int64, _P, _P]),
    'tgmx_tgcn_concat': (c_int32, [_P, c_int64, _P, _P, c_int32, c_int64, _P, _P]),
    'tgmx_tgcn_output': (c_int32, [_P, _P, _P, c_int64, _P, _P]),
    'tgmx_tgcn_forward': (c_int32, [_P, _P]),
    'tgmx_tgcn_gate_backward': (c_int32, [_P, _P, _P, _P, c_int64, _P, _P, _P, _P]),
    'tgmx_tgcn_reset_backward': (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int64, _P, _P, _P]),
    'tgmx_sgemm_tn_workspace_bytes': (c_size_t, [c_int64, c_int32, c_int32, c_int32]),
    'tgmx_sgemm_tn': (
        c_int32,
        [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int32, _P, _P],
    ),
    'tgmx_colsum': (c_int32, [_P, c_int64, c_int64, c_int32, _P, c_int32, _P, _P]),
    'tgmx_relu_mask': (c_int32, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P]),
    'tgmx_add_cols': (c_int32, [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P]),
    'tgmx_ln_backward': (c_int32, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int32, ctypes.c_float, c_int64, _P, c_int64, _P, c_int64, _P]),
    'tgmx_tgat_attn_backward': (
        c_int32,
        [_P, _P, _P, _P, c_int32, _P, c_int32, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int64, ctypes.c_float, c_int32, _P, _P, _P, _P, _P],
    ),
    'tgmx_dropout': (c_int32, [_P, c_int64, c_int64, c_int32, _P, _P, c_int64, _P]),
    'tgmx_ln_residual_concat': (c_int32, [_P, c_int64, _P, c_int64, _P, _P, c_int32, ctypes.c_float, _P, c_int32, c_int64, _P, c_int64, _P]),
}

TGAT_MAX_LAYERS = 4
E_UNSUPPORTED = -3  # TGMX_E_UNSUPPORTED


class Dropout(ctypes.Structure):
    """tgmx_dropout_t (include/tgm_amd.h)."""

    _fields_ = [('p', ctypes.c_float), ('seed', ctypes.c_uint64), ('stream', ctypes.c_uint64), ('row0', c_int64)]


def dropout_desc(p: float, seed: int, stream: int, row0: int = 0):
    """byref(tgmx_dropout_t) for an active dropout site, None (NULL) when p == 0."""
    if not p:
        return None
    d = Dropout(float(p), seed & 0xFFFFFFFFFFFFFFFF, stream & 0xFFFFFFFFFFFFFFFF, row0)
    return ctypes.byref(d)


class TgatLayer(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ('W_Q', 'W_K_t', 'W_V', 'W_O', 'b_O', 'ln_g', 'ln_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'qf_U', 'qf_v',
                                        'W_V_t16', 'W_O_t16', 'fc1_t16', 'fc2_t16', 'qf_lane', 'W_V_t16c')] + [
        (n, c_int32) for n in ('d', 'D', 'T', 'O', 'H', 'emb', 'emb_out')
    ] + [('ln_eps', ctypes.c_float)]


class TgatModel(ctypes.Structure):
    _fields_ = [('tw', c_void_p), ('tb', c_void_p), ('num_layers', c_int32), ('d0', c_int32), ('layers', TgatLayer * TGAT_MAX_LAYERS), ('drop', Dropout)]


class TgatHop(ctypes.Structure):
    _fields_ = [('seed_t', c_void_p), ('nbr_id', c_void_p), ('nbr_t', c_void_p), ('edge_x', c_void_p), ('k', c_int32), ('seed_keyed', c_int32),
                ('nbr_eid', c_void_p), ('edge_table', c_void_p)]  # fmt: skip


class TgatLayerGrads(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ('W_Q', 'W_KV', 'W_O', 'b_O', 'ln_g', 'ln_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')]


class TgatGrads(ctypes.Structure):
    _fields_ = [('tw', c_void_p), ('tb', c_void_p), ('layers', TgatLayerGrads * TGAT_MAX_LAYERS)]


PACK_MAX_JOBS = 32


class PackJob(ctypes.Structure):
    """tgmx_pack_job_t"""
    _fields_ = [('src', c_void_p), ('dst', c_void_p), ('src_ld', c_int64), ('dst_ld', c_int64), ('rows', c_int32), ('cols', c_int32),
                ('dst_rows', c_int32), ('dst_cols', c_int32), ('transpose', c_int32), ('reserved_', c_int32)]  # fmt: skip


class TgatLayerLayout(ctypes.Structure):
    _fields_ = [(n, c_int64) for n in ('R', 'rres', 'oattn', 'y', 'Q', 'qf', 'zbar', 'cat', 'h1', 'probs', 'out')] + [
        (n, c_int32) for n in ('Op', 'dhp', 'Cp', 'Kc', 'Ep')
    ]


class TgatLayout(ctypes.Structure):
    _fields_ = [('total_bytes', c_int64), ('z0', c_int64), ('level_rows', c_int64 * (TGAT_MAX_LAYERS + 1)),
                ('level_off', c_int64 * (TGAT_MAX_LAYERS + 2)), ('layers', TgatLayerLayout * TGAT_MAX_LAYERS),
                ('compact', c_int64 * (TGAT_MAX_LAYERS + 1))]  # fmt: skip


MAX_SEED_GROUPS = 8
MAX_HOPS = 8


class RecencyStep(ctypes.Structure):
    """tgmx_recency_step_t (include/tgm_amd.h)."""

    _fields_ = [
        ('ring', c_void_p), ('write_pos', c_void_p), ('ring_x', c_void_p),
        ('indptr', c_void_p), ('ev_lo', c_int64), ('ev_hi', c_int64),
        ('D', c_int32), ('B', c_int32), ('num_nodes', c_int32),
        ('n_groups', c_int32),
        ('grp_nid', c_void_p * MAX_SEED_GROUPS), ('grp_ts', c_void_p * MAX_SEED_GROUPS), ('grp_n', c_int64 * MAX_SEED_GROUPS),
        ('seed_nid0', c_void_p), ('seed_ts0', c_void_p), ('S0', c_int64),
        ('n_hops', c_int32), ('k', c_int32 * MAX_HOPS),
        ('out_nid', c_void_p * MAX_HOPS), ('out_ts', c_void_p * MAX_HOPS), ('out_x', c_void_p * MAX_HOPS),
        ('src', c_void_p), ('dst', c_void_p), ('ts', c_void_p), ('edge_x', c_void_p),
        ('n', c_int64), ('eid0', c_int64), ('directed', c_int32), ('key_wrap32', c_int32),
        ('scratch', c_void_p), ('status', c_void_p),
        ('timed_hop', c_int32), ('ev_start', c_void_p), ('ev_stop', c_void_p),
        ('ts_bound', c_int64),
        ('neg_group', c_int32), ('neg_low', c_int32), ('neg_high', c_int32),
        ('neg_seed', ctypes.c_uint64), ('neg_call', ctypes.c_uint64), ('neg_out', c_void_p), ('neg_time_out', c_void_p),
        ('guard_seed_errors', c_int32), ('sorted_ts', c_int32),
        ('out_valid', c_void_p * MAX_HOPS), ('out_valid_prev', c_void_p * MAX_HOPS),
        ('neg_index0', c_int64), ('csr_cursor', c_void_p), ('csr_x_by_pos', c_int32), ('out_eid', c_void_p * MAX_HOPS),
        ('defer', c_void_p), ('defer_ok', c_int32),
    ]  # fmt: skip


class PipelinePost(ctypes.Structure):
    """tgmx_pipeline_post_t (include/tgm_amd.h)."""

    _fields_ = [
        ('dedup', c_int32), ('dedup_neg', c_int32), ('dedup_nbr', c_int32), ('num_nodes', c_int32), ('dedup_ws', c_void_p), ('uniq_out', c_void_p),
        ('edge_hop', c_int32), ('edge_cap', c_int64), ('row_off', c_void_p), ('edge_index', c_void_p), ('edge_t', c_void_p), ('edge_x', c_void_p),
        ('dev_sizes', c_void_p), ('host_sizes', c_void_p), ('sizes_ready', c_void_p),
    ]  # fmt: skip


class TgnMemoryFwd(ctypes.Structure):
    """tgmx_tgn_memory_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('nodes', c_void_p), ('R', c_int64), ('memory', c_void_p), ('last_update', c_void_p), ('M', c_int32), ('num_nodes', c_int32),
        ('st_lo_s', c_void_p), ('st_cnt_s', c_void_p), ('st_lo_d', c_void_p), ('st_cnt_d', c_void_p),
        ('log_other', c_void_p), ('log_t', c_void_p), ('log_raw', c_void_p), ('D', c_int32),
        ('tw', c_void_p), ('tb', c_void_p), ('T', c_int32), ('mean', c_int32),
        ('W_ih', c_void_p), ('b_ih', c_void_p), ('W_hh', c_void_p), ('b_hh', c_void_p),
        ('ws_aggr', c_void_p), ('ws_h', c_void_p), ('ws_gi', c_void_p), ('ws_gh', c_void_p),
        ('out_mem', c_void_p), ('out_lu', c_void_p), ('assoc', c_void_p), ('stamp', c_int64),
    ]  # fmt: skip


class TgnStep(ctypes.Structure):
    """tgmx_tgn_step_t (include/tgm_amd.h)."""

    _fields_ = [
        ('mem', c_void_p), ('conv', c_void_p),
        ('src', c_void_p), ('dst', c_void_p), ('t', c_void_p), ('raw', c_void_p), ('n', c_int32),
        ('memory', c_void_p), ('last_update', c_void_p), ('reuse_status', c_void_p),
        ('log_base', c_int64), ('log_other', c_void_p), ('log_t', c_void_p), ('log_raw', c_void_p),
        ('st_lo_s', c_void_p), ('st_cnt_s', c_void_p), ('st_lo_d', c_void_p), ('st_cnt_d', c_void_p),
    ]  # fmt: skip


class TgcnFwd(ctypes.Structure):
    """tgmx_tgcn_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('x', c_void_p), ('N', c_int64), ('in_ch', c_int32), ('C', c_int32),
        ('src', c_void_p), ('dst', c_void_p), ('edge_w', c_void_p), ('E', c_int64), ('fill', ctypes.c_float), ('add_self_loops', c_int32),
        ('W3', c_void_p), ('b3', c_void_p),
        ('lin_w', c_void_p * 3), ('lin_b', c_void_p * 3),
        ('H', c_void_p),
        ('A', c_void_p), ('ldA', c_int64), ('norm_ws', c_void_p), ('xwt', c_void_p), ('G', c_void_p), ('cat', c_void_p), ('pre', c_void_p * 3),
        ('out', c_void_p), ('idx32', c_int32),
    ]  # fmt: skip


MIXER_MAX_LAYERS = 8  # TGMX_MIXER_MAX_LAYERS


class MixerLayer(ctypes.Structure):
    """tgmx_mixer_layer_t (include/tgm_amd.h)."""

    _fields_ = [(n, c_void_p) for n in ('tok_g', 'tok_b', 'tok_w1', 'tok_b1', 'tok_w2', 'tok_b2', 'ch_g', 'ch_b', 'ch_w1', 'ch_b1', 'ch_w2',
                                        'ch_b2')] + [('tok_hidden', c_int32), ('ch_hidden', c_int32)]  # fmt: skip


class GraphMixerFwd(ctypes.Structure):
    """tgmx_graphmixer_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('nbr_edge_x', c_void_p), ('seed_t', c_void_p), ('nbr_t', c_void_p), ('nbr_nids', c_void_p),
        ('seeds', c_void_p * 3), ('n_seeds', c_int64 * 3),
        ('tg_nbr', c_void_p), ('tg_lo', c_void_p), ('tg_cnt', c_void_p),
        ('node_x', c_void_p), ('num_nodes', c_int64), ('F', c_int32),
        ('S', c_int64), ('K', c_int32), ('D', c_int32), ('T', c_int32), ('E', c_int32), ('num_layers', c_int32), ('eps', ctypes.c_float),
        ('tw', c_void_p), ('tb', c_void_p), ('proj_w', c_void_p), ('proj_b', c_void_p), ('out_w', c_void_p), ('out_b', c_void_p),
        ('layers', MixerLayer * MIXER_MAX_LAYERS),
        ('x0', c_void_p), ('z', c_void_p), ('z1', c_void_p), ('y', c_void_p), ('h', c_void_p), ('cat', c_void_p),
        ('ldx0', c_int64), ('ldz', c_int64), ('ldh', c_int64), ('ldcat', c_int64),
        ('out', c_void_p),
    ]  # fmt: skip


class MixerLayerGrad(ctypes.Structure):
    """tgmx_mixer_layer_grad_t (include/tgm_amd.h)."""

    _fields_ = [(n, c_void_p) for n in ('tok_g', 'tok_b', 'tok_w1', 'tok_b1', 'tok_w2', 'tok_b2', 'ch_g', 'ch_b', 'ch_w1', 'ch_b1', 'ch_w2', 'ch_b2')]


class GraphMixerBwd(ctypes.Structure):
    """tgmx_graphmixer_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('S', c_int64), ('K', c_int32), ('D', c_int32), ('T', c_int32), ('E', c_int32), ('F', c_int32), ('num_layers', c_int32),
        ('eps', ctypes.c_float), ('drop_p', ctypes.c_float), ('drop_seed', ctypes.c_uint64), ('drop_stream', ctypes.c_uint64),
        ('g', c_void_p), ('ldg', c_int64),
        ('x0', c_void_p), ('save_z', c_void_p), ('save_z1', c_void_p), ('cat', c_void_p), ('nbr_nids', c_void_p),
        ('ldx0', c_int64), ('ldz', c_int64), ('ldh', c_int64), ('ldcat', c_int64),
        ('layers', MixerLayer * MIXER_MAX_LAYERS),
        ('ch_w1T', c_void_p * MIXER_MAX_LAYERS), ('ch_w2T', c_void_p * MIXER_MAX_LAYERS), ('out_wT', c_void_p),
        ('d_proj_w', c_void_p), ('d_proj_b', c_void_p), ('d_out_w', c_void_p), ('d_out_b', c_void_p),
        ('d_layers', MixerLayerGrad * MIXER_MAX_LAYERS),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


DYGFORMER_MAX_LAYERS = 8  # TGMX_DYGFORMER_MAX_LAYERS
DYGFORMER_MAX_SEQ = 2048  # slots per sequence (tgmx_dygformer_cooccurrence keeps both id sequences in LDS)
MHA_SMALL_MAX_TOKENS = 128  # tgmx_mha_small's envelope
MHA_SMALL_MAX_HEAD_DIM = 128


class DyGFormerLayer(ctypes.Structure):
    """tgmx_dygformer_layer_t (include/tgm_amd.h)."""

    _fields_ = [(n, c_void_p) for n in ('ln0_g', 'ln0_b', 'in_w', 'in_b', 'out_w', 'out_b', 'ln1_g', 'ln1_b', 'w1', 'b1', 'w2', 'b2')]


class DyGFormerFwd(ctypes.Structure):
    """tgmx_dygformer_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('node_x', c_void_p), ('num_nodes', c_int64),
        ('src', c_void_p), ('dst', c_void_p), ('edge_time', c_void_p), ('P', c_int64),
        ('nbr_nids', c_void_p), ('nbr_t', c_void_p), ('nbr_x', c_void_p), ('S', c_int64),
        ('src_rows', c_void_p), ('dst_rows', c_void_p),
        ('k', c_int32), ('dN', c_int32), ('dE', c_int32), ('dT', c_int32), ('C', c_int32), ('patch', c_int32), ('heads', c_int32), ('E', c_int32),
        ('num_layers', c_int32), ('eps', ctypes.c_float),
        ('tw', c_void_p), ('tb', c_void_p), ('co_w1', c_void_p), ('co_b1', c_void_p), ('co_w2', c_void_p), ('co_b2', c_void_p),
        ('proj_w', c_void_p * 4), ('proj_b', c_void_p * 4),
        ('out_w', c_void_p), ('out_b', c_void_p),
        ('layers', DyGFormerLayer * DYGFORMER_MAX_LAYERS),
        ('table', c_void_p), ('ch', c_void_p * 4), ('ldch', c_int64 * 4),
        ('x', c_void_p), ('y', c_void_p), ('x1', c_void_p), ('att', c_void_p), ('qkv', c_void_p), ('h', c_void_p), ('mean', c_void_p),
        ('ldx', c_int64), ('ldq', c_int64), ('ldh', c_int64),
        ('out', c_void_p),
    ]  # fmt: skip


class DyGFormerSave(ctypes.Structure):
    """tgmx_dygformer_save_t (include/tgm_amd.h)."""

    _fields_ = [(n, c_void_p) for n in ('counts', 'x', 'qkv', 'att', 'x1')]


class DyGFormerLayerGrad(ctypes.Structure):
    """tgmx_dygformer_layer_grad_t (include/tgm_amd.h)."""

    _fields_ = DyGFormerLayer._fields_


class DyGFormerLayerTr(ctypes.Structure):
    """tgmx_dygformer_layer_tr_t (include/tgm_amd.h)."""

    _fields_ = [(n, c_void_p) for n in ('in_wT', 'out_wT', 'w1T', 'w2T')]


class DyGFormerBwd(ctypes.Structure):
    """tgmx_dygformer_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('P', c_int64), ('S', c_int64),
        ('k', c_int32), ('dN', c_int32), ('dE', c_int32), ('dT', c_int32), ('C', c_int32), ('patch', c_int32), ('heads', c_int32), ('E', c_int32),
        ('num_layers', c_int32), ('eps', ctypes.c_float), ('drop_p', ctypes.c_float), ('drop_seed', ctypes.c_uint64), ('drop_stream', ctypes.c_uint64),
        ('src', c_void_p), ('dst', c_void_p), ('edge_time', c_void_p), ('nbr_nids', c_void_p), ('nbr_t', c_void_p), ('src_rows', c_void_p),
        ('dst_rows', c_void_p),
        ('g', c_void_p), ('ldg', c_int64),
        ('ch', c_void_p * 4), ('ldch', c_int64 * 4), ('counts', c_void_p), ('mean', c_void_p),
        ('save_x', c_void_p), ('save_qkv', c_void_p), ('save_att', c_void_p), ('save_x1', c_void_p), ('ldx', c_int64), ('ldq', c_int64), ('ldh', c_int64),
        ('layers', DyGFormerLayer * DYGFORMER_MAX_LAYERS),
        ('tr', DyGFormerLayerTr * DYGFORMER_MAX_LAYERS),
        ('out_wT', c_void_p), ('proj_wT', c_void_p * 4), ('tw', c_void_p), ('tb', c_void_p), ('co_w1', c_void_p), ('co_b1', c_void_p), ('co_w2T', c_void_p),
        ('d_tw', c_void_p), ('d_tb', c_void_p), ('d_co_w1', c_void_p), ('d_co_b1', c_void_p), ('d_co_w2', c_void_p), ('d_co_b2', c_void_p),
        ('d_proj_w', c_void_p * 4), ('d_proj_b', c_void_p * 4), ('d_out_w', c_void_p), ('d_out_b', c_void_p),
        ('d_layers', DyGFormerLayerGrad * DYGFORMER_MAX_LAYERS),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


class TconvFwd(ctypes.Structure):
    """tgmx_tconv_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('x', c_void_p), ('U', c_int64), ('in_ch', c_int32), ('last_update_local', c_void_p),
        ('src', c_void_p), ('tgt', c_void_p), ('t', c_void_p), ('msg', c_void_p), ('E', c_int64), ('D', c_int32), ('T', c_int32),
        ('tw', c_void_p), ('tb', c_void_p), ('W4', c_void_p), ('b4', c_void_p), ('W_edge', c_void_p), ('H', c_int32), ('C', c_int32),
        ('edge_attr', c_void_p), ('qkvs', c_void_p), ('eproj', c_void_p), ('order', c_void_p), ('seg_lo', c_void_p), ('seg_hi', c_void_p),
        ('sort_ws', c_void_p), ('sort_ws_bytes', c_size_t), ('status', c_void_p),
        ('tgt_count', c_void_p), ('cursor', c_void_p), ('order_big', c_void_p),
    ]  # fmt: skip


SEED_SRC, SEED_DST, SEED_NEG = 0, 1, 2


class Pipeline(ctypes.Structure):
    """tgmx_pipeline_t (include/tgm_amd.h)."""

    _fields_ = [
        ('src', c_void_p), ('dst', c_void_p), ('ts', c_void_p), ('edge_x', c_void_p), ('num_edges', c_int64),
        ('rank', c_int32), ('world', c_int32), ('n_roles', c_int32), ('seed_role', c_int32 * MAX_SEED_GROUPS),
        ('neg_low', c_int32), ('neg_high', c_int32), ('neg_seed', ctypes.c_uint64),
        ('update', c_int32), ('reserved0', c_int32), ('step', RecencyStep),
    ]  # fmt: skip


class PipelineOut(ctypes.Structure):
    """tgmx_pipeline_out_t (include/tgm_amd.h)."""

    _fields_ = [
        ('neg', c_void_p), ('neg_time', c_void_p), ('seed_nid0', c_void_p), ('seed_ts0', c_void_p),
        ('out_nid', c_void_p * MAX_HOPS), ('out_ts', c_void_p * MAX_HOPS), ('out_x', c_void_p * MAX_HOPS),
        ('timed_hop', c_int32), ('ev_start', c_void_p), ('ev_stop', c_void_p),
        ('out_valid', c_void_p * MAX_HOPS), ('out_valid_prev', c_void_p * MAX_HOPS), ('out_eid', c_void_p * MAX_HOPS),
    ]  # fmt: skip


ACCOUNTING_PARTIALS = 1024
SIGNATURES['tgmx_lookup_accounting'] = (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P])
SIGNATURES['tgmx_uniform_lookup_csr'] = (c_int32, [_P, _P, _P, c_int32, _P, c_int64, c_int32, c_int64, c_int32, c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                                   _P, _P, _P, _P, _P])
SIGNATURES['tgmx_ring_update_scratch_bytes'] = (c_size_t, [c_int64, c_int32])
SIGNATURES['tgmx_defer_create'] = (c_void_p, [c_int32, c_int32])
SIGNATURES['tgmx_defer_destroy'] = (None, [_P])
SIGNATURES['tgmx_defer_pending'] = (c_int32, [_P])
SIGNATURES['tgmx_defer_count'] = (c_int64, [_P])
SIGNATURES['tgmx_defer_flush'] = (c_int32, [_P, _P])
SIGNATURES['tgmx_set_fused_rows'] = (c_int32, [c_int32])
SIGNATURES['tgmx_set_fused_order'] = (c_int32, [c_int32])
SIGNATURES['tgmx_fused_row_order'] = (c_int32, [c_int64, c_int32, c_int32, _P, c_int32, _P])
SIGNATURES['tgmx_tgn_gru_gate_backward'] = (c_int32, [_P, _P, _P, _P, c_int32, c_int64, _P, _P, _P])
SIGNATURES['tgmx_tgn_aggregate_backward'] = (c_int32, [c_int64, _P, _P, _P, _P, _P, _P, c_int32, c_int32, _P, _P, c_int32, c_int32, _P, _P, _P])
SIGNATURES['tgmx_tconv_edge_attr_backward'] = (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int64, _P, _P])
SIGNATURES['tgmx_tconv_attend_backward'] = (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, ctypes.c_float, _P, _P, _P, _P, _P, _P, _P])
SIGNATURES['tgmx_group_ids'] = (c_int32, [_P, c_int32, _P, _P, _P, _P, _P, _P])
SIGNATURES['tgmx_group_ids_workspace_bytes'] = (c_size_t, [c_int64])
SIGNATURES['tgmx_group_ids_large'] = (c_int32, [_P, c_int64, _P, _P, _P, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_random_negatives'] = (c_int32, [c_int32, c_int32, c_int64, ctypes.c_uint64, ctypes.c_uint64, _P, _P, c_int64, _P, _P])
SIGNATURES['tgmx_random_negatives_at'] = (c_int32, [c_int32, c_int32, c_int64, ctypes.c_uint64, ctypes.c_uint64, c_int64, _P, _P, c_int64, _P, _P])
SIGNATURES['tgmx_unique_ids_workspace_bytes'] = (c_size_t, [c_int32])
SIGNATURES['tgmx_unique_ids'] = (c_int32, [_P, _P, c_int32, c_int32, _P, _P, _P, _P, _P])
SIGNATURES['tgmx_csr_build_workspace_bytes'] = (c_size_t, [c_int64, c_int32, c_int32])
SIGNATURES['tgmx_csr_build'] = (c_int32, [_P, _P, _P, c_int64, c_int32, _P, c_int64, c_int32, _P, _P, _P, c_size_t, _P, _P])
SIGNATURES['tgmx_recency_step'] = (c_int32, [ctypes.POINTER(RecencyStep), _P])
SIGNATURES['tgmx_recency_step_plan'] = (c_int32, [ctypes.POINTER(RecencyStep)])
SIGNATURES['tgmx_pipeline_step'] = (c_int32, [ctypes.POINTER(Pipeline), c_int64, c_int64, ctypes.c_uint64, ctypes.POINTER(PipelineOut), ctypes.POINTER(PipelinePost), _P])
SIGNATURES['tgmx_event_synchronize'] = (c_int32, [_P])
SIGNATURES['tgmx_event_create_sync'] = (c_int32, [ctypes.POINTER(c_void_p)])
SIGNATURES['tgmx_event_record'] = (c_int32, [_P, _P])
SIGNATURES['tgmx_stream_wait_event'] = (c_int32, [_P, _P])
SIGNATURES['tgmx_stream_handoff'] = (c_int32, [_P, _P, _P])
SIGNATURES['tgmx_worker_create'] = (c_int32, [ctypes.POINTER(c_void_p)])
SIGNATURES['tgmx_worker_destroy'] = (c_int32, [_P])
SIGNATURES['tgmx_worker_pipeline_step'] = (c_int32, [_P, ctypes.POINTER(Pipeline), c_int64, c_int64, ctypes.c_uint64, ctypes.POINTER(PipelineOut),
                                                     ctypes.POINTER(PipelinePost), _P, _P, _P, ctypes.POINTER(ctypes.c_uint64)])
SIGNATURES['tgmx_worker_wait'] = (c_int32, [_P, ctypes.c_uint64])
SIGNATURES['tgmx_slice'] = (c_int32, [_P, c_int64, c_int32, c_int64, c_int32, c_int64, c_int64, c_int64, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)])
SIGNATURES['tgmx_discretize_workspace_bytes'] = (c_size_t, [c_int64])
SIGNATURES['tgmx_discretize_keep'] = (c_int32, [_P, _P, _P, c_int64, ctypes.c_double, _P, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_tgn_memory_forward'] = (c_int32, [ctypes.POINTER(TgnMemoryFwd), _P])
SIGNATURES['tgmx_tconv_forward'] = (c_int32, [ctypes.POINTER(TconvFwd), _P])
SIGNATURES['tgmx_tgn_step'] = (c_int32, [ctypes.POINTER(TgnStep), _P])
SIGNATURES['tgmx_segment_sort_workspace_bytes'] = (c_size_t, [c_int64])
SIGNATURES['tgmx_segment_sort'] = (c_int32, [_P, c_int64, c_int32, _P, _P, _P, _P, c_size_t, _P, _P])
SIGNATURES['tgmx_tgat_tile16_floats'] = (c_size_t, [c_int32, c_int32])
SIGNATURES['tgmx_tgat_tile16'] = (c_int32, [_P, c_int64, c_int32, c_int32, _P, _P])
SIGNATURES['tgmx_pack2d'] = (c_int32, [ctypes.POINTER(PackJob), c_int32, _P])

SIGNATURES['tgmx_pair_dedup_workspace_bytes'] = (c_size_t, [c_int64])
SIGNATURES['tgmx_pair_dedup'] = (c_int32, [_P, _P, c_int64, _P, _P, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_tgat_layout'] = (c_int32, [ctypes.POINTER(TgatModel), c_int64, ctypes.POINTER(TgatHop), c_int32, ctypes.POINTER(TgatLayout)])
SIGNATURES['tgmx_tgat_workspace_bytes'] = (c_size_t, [ctypes.POINTER(TgatModel), c_int64, ctypes.POINTER(TgatHop)])
SIGNATURES['tgmx_tgat_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(TgatModel), ctypes.POINTER(TgatLayout), ctypes.POINTER(TgatHop)])
SIGNATURES['tgmx_tgat_backward'] = (c_int32, [ctypes.POINTER(TgatModel), ctypes.POINTER(TgatLayout), ctypes.POINTER(TgatHop), _P, _P, c_int64,
                                              ctypes.POINTER(Dropout), ctypes.POINTER(TgatGrads), _P, c_size_t, _P])  # fmt: skip
SIGNATURES['tgmx_tgat_forward'] = (
    c_int32,
    [ctypes.POINTER(TgatModel), _P, c_int64, _P, c_int64, ctypes.POINTER(TgatHop), _P, c_size_t, c_int32, _P, _P],
)

SIGNATURES['tgmx_sgemm_nt_ep'] = (c_int32, [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_time_gap_workspace_bytes'] = (c_size_t, [c_int64])
SIGNATURES['tgmx_time_gap_group'] = (c_int32, [_P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_size_t, _P, _P, _P, _P])
SIGNATURES['tgmx_mixer_prologue'] = (c_int32, [_P, _P, _P, c_int64, c_int32, c_int32, _P, _P, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_mixer_token'] = (
    c_int32,
    [_P, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, _P, c_int32, _P, _P, _P, _P, ctypes.c_float, _P, _P, c_int64, _P],
)
SIGNATURES['tgmx_mixer_tail'] = (
    c_int32,
    [_P, c_int64, c_int64, c_int32, c_int32, _P, _P, c_int64, c_int32, _P, _P, _P, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P],
)
SIGNATURES['tgmx_graphmixer_forward'] = (c_int32, [ctypes.POINTER(GraphMixerFwd), _P])
SIGNATURES['tgmx_mixer_train_supported'] = (c_int32, [c_int32, c_int32, c_int32])
SIGNATURES['tgmx_mixer_token_train'] = (c_int32, SIGNATURES['tgmx_mixer_token'][1][:-1] + [_P, _P, _P])
SIGNATURES['tgmx_graphmixer_forward_train'] = (c_int32, [ctypes.POINTER(GraphMixerFwd), _P, _P, _P, _P])
SIGNATURES['tgmx_mixer_channel_norm'] = (c_int32, [_P, c_int64, c_int64, c_int32, _P, _P, ctypes.c_float, _P, c_int64, _P])
SIGNATURES['tgmx_mixer_gelu_backward'] = (c_int32, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P, _P])
SIGNATURES['tgmx_mixer_tail_backward'] = (c_int32, [_P, c_int64, _P, c_int64, c_int32, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_mixer_token_backward'] = (c_int32, [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, _P, c_int32, _P, ctypes.c_float, _P,
                                                     c_int64, _P, c_int64, _P, _P, _P])  # fmt: skip
SIGNATURES['tgmx_graphmixer_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(GraphMixerBwd)])
SIGNATURES['tgmx_graphmixer_backward'] = (c_int32, [ctypes.POINTER(GraphMixerBwd), _P])
SIGNATURES['tgmx_dygformer_cooccurrence'] = (c_int32, [_P, _P, c_int64, _P, c_int64, c_int32, _P, _P, _P, _P, _P, _P, c_int32, _P, _P, _P, c_int64, _P])
SIGNATURES['tgmx_dygformer_prologue'] = (
    c_int32,
    [_P, c_int64, c_int32, _P, _P, _P, c_int64, _P, _P, _P, c_int64, c_int32, c_int32, _P, _P, _P, _P, c_int32, _P, c_int64, _P, c_int64, _P, c_int64, _P],
)
SIGNATURES['tgmx_layernorm_rows'] = (c_int32, [_P, c_int64, c_int64, c_int32, _P, _P, ctypes.c_float, _P, c_int64, _P])
SIGNATURES['tgmx_mha_small'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_dygformer_tail'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P, _P, c_int32, _P, _P])
SIGNATURES['tgmx_dygformer_layer'] = (
    c_int32,
    [ctypes.POINTER(DyGFormerLayer), c_int64, c_int32, c_int32, c_int32, ctypes.c_float, _P, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P],
)
SIGNATURES['tgmx_dygformer_forward'] = (c_int32, [ctypes.POINTER(DyGFormerFwd), _P])
SIGNATURES['tgmx_mha_small_train_supported'] = (c_int32, [c_int32, c_int32])
SIGNATURES['tgmx_mha_small_train'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, c_int32, _P, c_int64, _P, _P])
SIGNATURES['tgmx_mha_small_backward'] = (c_int32, [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_int32, _P, _P, _P])
SIGNATURES['tgmx_dygformer_layer_train'] = (
    c_int32,
    [ctypes.POINTER(DyGFormerLayer), c_int64, c_int32, c_int32, c_int32, ctypes.c_float, _P, _P, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P],
)
SIGNATURES['tgmx_dygformer_forward_train'] = (c_int32, [ctypes.POINTER(DyGFormerFwd), ctypes.POINTER(DyGFormerSave), _P, _P])
SIGNATURES['tgmx_dygformer_mean_backward'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_dygformer_time_backward'] = (c_int32, [_P, c_int64, _P, _P, _P, c_int64, _P, _P, c_int64, c_int32, _P, _P, _P, _P, c_int32, _P, _P])
SIGNATURES['tgmx_dygformer_cooccurrence_backward_workspace_bytes'] = (c_size_t, [c_int64, c_int32, c_int32])
SIGNATURES['tgmx_dygformer_cooccurrence_backward'] = (c_int32, [_P, _P, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_dygformer_layer_backward_workspace_bytes'] = (c_size_t, [c_int64, c_int32, c_int32, c_int64, c_int64, c_int64])
SIGNATURES['tgmx_dygformer_layer_backward'] = (
    c_int32,
    [ctypes.POINTER(DyGFormerLayer), ctypes.POINTER(DyGFormerLayerTr), ctypes.POINTER(DyGFormerLayerGrad), c_int64, c_int32, c_int32, c_int32,
     ctypes.c_float, _P, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P],
)  # fmt: skip
SIGNATURES['tgmx_dygformer_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(DyGFormerBwd)])
SIGNATURES['tgmx_dygformer_backward'] = (c_int32, [ctypes.POINTER(DyGFormerBwd), _P])

TPNET_MAX_LEVELS = 8  # TGMX_TPNET_MAX_LEVELS
TPNET_PAIR_MAX_LEVELS = 4  # tgmx_tpnet_pair_features' envelope (tables per side)
TPNET_HEAD_EMPTY = 0x7F7F7F7F  # TGMX_TPNET_HEAD_EMPTY


class TPNetTables(ctypes.Structure):
    """tgmx_tpnet_tables_t (include/tgm_amd.h)."""

    _fields_ = [('P', c_void_p * TPNET_MAX_LEVELS), ('levels', c_int32), ('dim', c_int32), ('num_nodes', c_int64)]


class TPNetFwd(ctypes.Structure):
    """tgmx_tpnet_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('node_x', c_void_p), ('num_nodes', c_int64),
        ('src', c_void_p), ('dst', c_void_p), ('edge_time', c_void_p), ('B', c_int64),
        ('nbr_nids', c_void_p), ('nbr_t', c_void_p), ('nbr_x', c_void_p), ('S', c_int64),
        ('rows', c_void_p),
        ('k', c_int32), ('dN', c_int32), ('dE', c_int32), ('dT', c_int32), ('E', c_int32), ('num_layers', c_int32), ('rp_concat', c_int32),
        ('rp_scale', c_int32), ('rp_out_dim', c_int32), ('eps', ctypes.c_float),
        ('tables', TPNetTables),
        ('rp_w1', c_void_p), ('rp_b1', c_void_p), ('rp_w2', c_void_p), ('rp_b2', c_void_p),
        ('tw', c_void_p), ('tb', c_void_p), ('proj_w0', c_void_p), ('proj_b0', c_void_p), ('proj_w2', c_void_p), ('proj_b2', c_void_p),
        ('layers', MixerLayer * MIXER_MAX_LAYERS),
        ('feat', c_void_p), ('feat_h', c_void_p), ('pf', c_void_p), ('x0', c_void_p), ('hp', c_void_p), ('z', c_void_p), ('z1', c_void_p),
        ('y', c_void_p), ('h', c_void_p),
        ('ldf', c_int64), ('ldfh', c_int64), ('ldx0', c_int64), ('ldhp', c_int64), ('ldz', c_int64), ('ldh', c_int64),
        ('out', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_tpnet_update'] = (c_int32, [ctypes.POINTER(TPNetTables), _P, _P, _P, c_int64, ctypes.c_double, _P, c_int32, _P, _P, _P, _P])
SIGNATURES['tgmx_tpnet_pair_features'] = (c_int32, [ctypes.POINTER(TPNetTables), _P, _P, c_int64, c_int32, _P, _P, c_int64, c_int64, c_int32, c_int32,
                                                    _P, c_int64, _P])
SIGNATURES['tgmx_tpnet_tokens'] = (c_int32, [_P, c_int64, c_int32, _P, c_int64, _P, _P, _P, c_int64, c_int32, c_int32, _P, _P, _P, c_int32, _P, c_int64,
                                             c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_tpnet_token_mix'] = SIGNATURES['tgmx_mixer_token']
SIGNATURES['tgmx_tpnet_mean'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_tpnet_forward'] = (c_int32, [ctypes.POINTER(TPNetFwd), _P])


class TPNetSave(ctypes.Structure):
    """tgmx_tpnet_save_t (include/tgm_amd.h)."""

    _fields_ = [('z', c_void_p), ('z1', c_void_p), ('lg', c_void_p)]


class TPNetBwd(ctypes.Structure):
    """tgmx_tpnet_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('B', c_int64), ('k', c_int32), ('dN', c_int32), ('dE', c_int32), ('dT', c_int32), ('E', c_int32), ('od', c_int32), ('num_layers', c_int32),
        ('eps', ctypes.c_float), ('drop_p', ctypes.c_float), ('drop_seed', ctypes.c_uint64), ('drop_stream', ctypes.c_uint64),
        ('g', c_void_p), ('ldg', c_int64),
        ('feat', c_void_p), ('feat_h', c_void_p), ('x0', c_void_p), ('hp', c_void_p), ('save_z', c_void_p), ('save_z1', c_void_p), ('lg', c_void_p),
        ('ldf', c_int64), ('ldfh', c_int64), ('ldx0', c_int64), ('ldhp', c_int64), ('ldz', c_int64), ('ldh', c_int64),
        ('tw', c_void_p), ('tb', c_void_p),
        ('layers', MixerLayer * MIXER_MAX_LAYERS),
        ('ch_w1T', c_void_p * MIXER_MAX_LAYERS), ('ch_w2T', c_void_p * MIXER_MAX_LAYERS),
        ('proj_w2T', c_void_p), ('w0T_time', c_void_p), ('w0T_pair0', c_void_p), ('w0T_pair1', c_void_p), ('rp_w2T', c_void_p),
        ('d_tw', c_void_p), ('d_tb', c_void_p), ('d_proj_w0', c_void_p), ('d_proj_b0', c_void_p), ('d_proj_w2', c_void_p), ('d_proj_b2', c_void_p),
        ('d_rp_w1', c_void_p), ('d_rp_b1', c_void_p), ('d_rp_w2', c_void_p), ('d_rp_b2', c_void_p),
        ('d_layers', MixerLayerGrad * MIXER_MAX_LAYERS),
        ('d_tok', c_void_p * MIXER_MAX_LAYERS),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


SIGNATURES['tgmx_tpnet_train_supported'] = (c_int32, [c_int32, c_int32, c_int32])
SIGNATURES['tgmx_tpnet_token_mix_train'] = SIGNATURES['tgmx_mixer_token_train']
SIGNATURES['tgmx_tpnet_forward_train'] = (c_int32, [ctypes.POINTER(TPNetFwd), ctypes.POINTER(TPNetSave), _P, _P])
SIGNATURES['tgmx_tpnet_mean_backward'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P])
SIGNATURES['tgmx_tpnet_time_backward'] = (c_int32, [_P, c_int64, _P, c_int64, _P, _P, c_int32, _P, _P])
SIGNATURES['tgmx_tpnet_token_backward'] = SIGNATURES['tgmx_mixer_token_backward']
SIGNATURES['tgmx_tpnet_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(TPNetBwd)])
SIGNATURES['tgmx_tpnet_backward'] = (c_int32, [ctypes.POINTER(TPNetBwd), _P])


class NCNFwd(ctypes.Structure):
    """tgmx_ncn_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('x', c_void_p), ('N', c_int64),
        ('C', c_int32), ('k', c_int32), ('H', c_int32), ('out_ch', c_int32), ('decay', c_int32), ('dup_all', c_int32),
        ('edge_index', c_void_p), ('ei_stride', c_int64), ('E', c_int64), ('ei_is64', c_int32), ('have_adj', c_int32),
        ('tar', c_void_p), ('tar_stride', c_int64), ('B', c_int64), ('tar_is64', c_int32), ('reserved_', c_int32),
        ('last_update', c_void_p), ('edge_time', c_void_p),
        ('w1', c_void_p), ('b1', c_void_p), ('w2', c_void_p), ('b2', c_void_p),
        ('indptr', c_void_p), ('cols', c_void_p), ('adj_ws', c_void_p), ('adj_ws_bytes', c_size_t),
        ('last', c_void_p),
        ('xs', c_void_p), ('h', c_void_p), ('ldxs', c_int64), ('ldh', c_int64),
        ('out', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_ncn_adj_workspace_bytes'] = (c_size_t, [c_int64])
SIGNATURES['tgmx_ncn_adj_build'] = (c_int32, [_P, c_int32, c_int64, c_int64, c_int64, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_ncn_cn_emb'] = (c_int32, [_P, c_int64, c_int32, c_int32, _P, _P, _P, c_int32, c_int64, c_int64, _P, _P, _P, _P, c_int64, _P])
SIGNATURES['tgmx_ncn_forward'] = (c_int32, [ctypes.POINTER(NCNFwd), _P])
SIGNATURES['tgmx_ncn8_lds_max_nodes'] = (c_int32, [])
SIGNATURES['tgmx_ncn8_workspace_bytes'] = (c_size_t, [c_int64, c_int64])
SIGNATURES['tgmx_ncn8_cn_emb'] = (c_int32, [_P, c_int64, c_int32, _P, _P, _P, c_int32, c_int64, c_int64, _P, _P, _P, _P, c_int64, _P, c_size_t, c_int32,
                                            _P])  # fmt: skip
SIGNATURES['tgmx_ncn8_forward'] = (c_int32, [ctypes.POINTER(NCNFwd), _P, c_size_t, _P])


class NcnBwd(ctypes.Structure):
    """tgmx_ncn_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('fwd', NCNFwd),
        ('dout', c_void_p), ('lddout', c_int64),
        ('d_x', c_void_p), ('d_w1', c_void_p), ('d_b1', c_void_p), ('d_w2', c_void_p), ('d_b2', c_void_p),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


SIGNATURES['tgmx_ncn_dx_workspace_bytes'] = (c_size_t, [c_int64, c_int64, c_int64, c_int32])
SIGNATURES['tgmx_ncn_dx'] = (c_int32, [_P, c_int64, c_int32, c_int32, _P, _P, c_int64, _P, c_int32, c_int64, c_int64, _P, _P, _P, _P, c_int64, _P,
                                       _P, c_size_t, _P])  # fmt: skip
SIGNATURES['tgmx_ncn_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(NcnBwd)])
SIGNATURES['tgmx_ncn_backward'] = (c_int32, [ctypes.POINTER(NcnBwd), _P])


class EdgeBank(ctypes.Structure):
    """tgmx_edgebank_t (include/tgm_amd.h)."""

    _fields_ = [
        ('table', c_void_p), ('stamp', c_void_p), ('capacity', c_int64),
        ('state', c_void_p),
        ('fixed', c_int32), ('reserved_', c_int32),
        ('pos_prob', ctypes.c_double),
        ('arrivals', c_int64),
        ('status', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_edgebank_state_bytes'] = (c_size_t, [])
SIGNATURES['tgmx_edgebank_update'] = (c_int32, [ctypes.POINTER(EdgeBank), _P, c_int32, _P, c_int32, _P, c_int32, c_int64, _P])
SIGNATURES['tgmx_edgebank_query'] = (c_int32, [ctypes.POINTER(EdgeBank), _P, c_int32, _P, c_int32, _P, c_int32, _P, c_int64, c_int64, c_int64, _P, c_int32, _P])
SIGNATURES['tgmx_edgebank_rehash'] = (c_int32, [ctypes.POINTER(EdgeBank), ctypes.POINTER(EdgeBank), _P, _P])


class TCoMem(ctypes.Structure):
    """tgmx_tcomem_t (include/tgm_amd.h)."""

    _fields_ = [
        ('ring', c_void_p), ('pos', c_void_p), ('len', c_void_p), ('popularity', c_void_p),
        ('table', c_void_p), ('capacity', c_int64),
        ('state', c_void_p),
        ('num_nodes', c_int64), ('k', c_int32), ('reserved_', c_int32),
        ('co_occurrence_weight', ctypes.c_double),
        ('status', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_tcomem_state_bytes'] = (c_size_t, [])
SIGNATURES['tgmx_tcomem_update'] = (c_int32, [ctypes.POINTER(TCoMem), _P, c_int32, _P, c_int32, _P, c_int32, c_int64, _P])
SIGNATURES['tgmx_tcomem_query'] = (c_int32, [ctypes.POINTER(TCoMem), _P, c_int32, _P, c_int32, _P, c_int32, _P, c_int64, c_int64, c_int64, _P, c_int32, _P])
SIGNATURES['tgmx_tcomem_rehash'] = (c_int32, [ctypes.POINTER(TCoMem), ctypes.POINTER(TCoMem), _P, _P])


class CtanFwd(ctypes.Structure):
    """tgmx_ctan_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('node_x', c_void_p), ('U', c_int64), ('in_ch', c_int32), ('M', c_int32), ('last_update', c_void_p),
        ('src', c_void_p), ('tgt', c_void_p), ('t', c_void_p), ('msg', c_void_p), ('E', c_int64), ('D', c_int32), ('T', c_int32),
        ('tw', c_void_p), ('tb', c_void_p), ('W_x', c_void_p), ('b_x', c_void_p), ('W4', c_void_p), ('b4', c_void_p), ('W_edge', c_void_p),
        ('num_iters', c_int32), ('epsilon', ctypes.c_float), ('mean_delta_t', ctypes.c_float), ('std_delta_t', ctypes.c_float),
        ('edge_attr', c_void_p), ('eproj', c_void_p), ('x', c_void_p), ('qkvs', c_void_p),
        ('src_ok', c_void_p), ('order', c_void_p), ('seg_lo', c_void_p), ('seg_hi', c_void_p),
        ('sort_ws', c_void_p), ('sort_ws_bytes', c_size_t), ('status', c_void_p),
        ('out', c_void_p),
        ('x_save', c_void_p),
    ]  # fmt: skip


class CtanBwd(ctypes.Structure):
    """tgmx_ctan_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('U', c_int64), ('E', c_int64), ('in_ch', c_int32), ('M', c_int32), ('D', c_int32), ('T', c_int32), ('num_iters', c_int32),
        ('epsilon', ctypes.c_float), ('mean_delta_t', ctypes.c_float), ('std_delta_t', ctypes.c_float),
        ('g', c_void_p), ('ldg', c_int64), ('out', c_void_p), ('x_save', c_void_p), ('node_x', c_void_p),
        ('last_update', c_void_p), ('t', c_void_p), ('tw', c_void_p), ('tb', c_void_p),
        ('W4', c_void_p), ('b4', c_void_p), ('W4T', c_void_p), ('WxT', c_void_p), ('WeT', c_void_p),
        ('edge_attr', c_void_p), ('eproj', c_void_p), ('src_ok', c_void_p), ('order', c_void_p), ('seg_lo', c_void_p), ('seg_hi', c_void_p),
        ('d_W4', c_void_p), ('d_b4', c_void_p), ('d_W', c_void_p), ('d_Wx', c_void_p), ('d_bx', c_void_p), ('d_node_x', c_void_p),
        ('d_Wedge', c_void_p), ('d_time', c_void_p),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


SIGNATURES['tgmx_ctan_out_backward'] = (c_int32, [_P, c_int64, _P, c_int64, c_int32, _P, _P])
SIGNATURES['tgmx_ctan_attend_backward'] = (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, ctypes.c_float, ctypes.c_float, _P, _P, _P, _P, _P, _P,
                                                     c_int32, _P])  # fmt: skip
SIGNATURES['tgmx_ctan_source_backward'] = (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, _P])
SIGNATURES['tgmx_ctan_edge_attr_backward'] = (c_int32, [_P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int64, ctypes.c_float, ctypes.c_float, _P, _P])
SIGNATURES['tgmx_ctan_antisym_grad'] = (c_int32, [_P, c_int32, _P, _P])
SIGNATURES['tgmx_ctan_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(CtanBwd)])
SIGNATURES['tgmx_ctan_backward'] = (c_int32, [ctypes.POINTER(CtanBwd), _P])
SIGNATURES['tgmx_ctan_memory_update'] = (c_int32, [_P, c_int32, _P, c_int32, _P, c_int64, _P, _P, c_int64, c_int32, c_int64, _P, _P, _P, _P, _P, _P])
SIGNATURES['tgmx_ctan_attend'] = (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, ctypes.c_float, _P, _P, _P, ctypes.c_float, c_int32, _P])
SIGNATURES['tgmx_ctan_forward'] = (c_int32, [ctypes.POINTER(CtanFwd), _P])

CHEB_NORM = {None: 0, 'sym': 1, 'rw': 2}  # TGMX_CHEB_NORM_*


class GclstmFwd(ctypes.Structure):
    """tgmx_gclstm_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('x', c_void_p), ('N', c_int64), ('in_ch', c_int32), ('C', c_int32), ('K', c_int32), ('normalization', c_int32),
        ('src', c_void_p), ('dst', c_void_p), ('edge_w', c_void_p), ('E', c_int64), ('idx64', c_int32), ('lambda_max', ctypes.c_float),
        ('lambda_ptr', c_void_p),
        ('W', c_void_p), ('b', c_void_p), ('ldw', c_int64),
        ('H', c_void_p), ('Cprev', c_void_p),
        ('indptr', c_void_p), ('cols', c_void_p), ('vals', c_void_p), ('diag', c_void_p),
        ('lap_ws', c_void_p), ('lap_ws_bytes', c_size_t), ('skipped', c_void_p), ('prop_ws', c_void_p), ('prop_ws_floats', c_size_t),
        ('op', c_void_p), ('ldop', c_int64), ('pre', c_void_p),
        ('H_out', c_void_p), ('C_out', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_cheb_workspace_bytes'] = (c_size_t, [c_int64, c_int64])
SIGNATURES['tgmx_cheb_laplacian'] = (c_int32, [_P, _P, c_int32, _P, c_int64, c_int64, c_int32, ctypes.c_float, _P, _P, _P, _P, _P, _P, c_size_t, _P, _P])
SIGNATURES['tgmx_cheb_propagate_scratch_floats'] = (c_size_t, [c_int64, c_int32])
SIGNATURES['tgmx_cheb_propagate'] = (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, c_int64, _P, c_int64, ctypes.c_float, ctypes.c_float, _P, c_int64, c_int64, _P, c_size_t, _P])
SIGNATURES['tgmx_gclstm_forward'] = (c_int32, [ctypes.POINTER(GclstmFwd), _P])


class GclstmBwd(ctypes.Structure):
    """tgmx_gclstm_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('N', c_int64), ('in_ch', c_int32), ('C', c_int32), ('K', c_int32), ('normalization', c_int32),
        ('op', c_void_p), ('ldop', c_int64), ('pre', c_void_p), ('Cprev', c_void_p),
        ('dH_out', c_void_p), ('lddh', c_int64), ('dC_out', c_void_p), ('lddc', c_int64),
        ('WT', c_void_p), ('ldwt', c_int64),
        ('src', c_void_p), ('dst', c_void_p), ('edge_w', c_void_p), ('E', c_int64), ('idx64', c_int32), ('lambda_max', ctypes.c_float),
        ('lambda_ptr', c_void_p),
        ('d_W', c_void_p), ('d_lins', c_void_p), ('d_b', c_void_p), ('d_conv_bias', c_void_p),
        ('d_x', c_void_p), ('d_H', c_void_p), ('d_Cprev', c_void_p),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


SIGNATURES['tgmx_gclstm_gate_backward'] = (c_int32, [_P, _P, c_int64, c_int32, _P, c_int64, _P, c_int64, _P, _P, _P])
SIGNATURES['tgmx_cheb_laplacian_t'] = SIGNATURES['tgmx_cheb_laplacian']
SIGNATURES['tgmx_cheb_propagate2'] = (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, c_int64, _P, c_int64, _P, c_int64, ctypes.c_float, ctypes.c_float,
                                                ctypes.c_float, _P, c_int64, c_int64, _P, c_size_t, _P])  # fmt: skip
SIGNATURES['tgmx_cheb_clenshaw'] = (c_int32, [_P, _P, _P, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int64, c_int64, _P, c_size_t, _P])
SIGNATURES['tgmx_gclstm_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(GclstmBwd)])
SIGNATURES['tgmx_gclstm_backward'] = (c_int32, [ctypes.POINTER(GclstmBwd), _P])

GCN_EPI = {'none': 0, 'relu': 1, 'tau': 2}  # TGMX_GCN_EPI_*
ROLAND_UPDATE = {'moving': 0, 'learnable': 0, None: 0, 'mlp': 1, 'gru': 2}  # TGMX_ROLAND_*


class RolandFwd(ctypes.Structure):
    """tgmx_roland_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('x', c_void_p), ('N', c_int64), ('in_ch', c_int32), ('C', c_int32), ('update', c_int32), ('add_self_loops', c_int32),
        ('src', c_void_p), ('dst', c_void_p), ('E', c_int64), ('idx64', c_int32), ('fill', ctypes.c_float),
        ('conv_w', c_void_p * 2), ('ldw', c_int64 * 2), ('conv_b', c_void_p * 2),
        ('tau', ctypes.c_float), ('tau_ptr', c_void_p),
        ('prev', c_void_p * 2), ('ldp', c_int64), ('prev_copy', c_void_p * 2),
        ('mlp_w', c_void_p * 2), ('mlp_b', c_void_p * 2),
        ('w_ih', c_void_p * 2), ('w_hh', c_void_p * 2), ('b_ih', c_void_p * 2), ('b_hh', c_void_p * 2),
        ('indptr', c_void_p), ('cols', c_void_p), ('vals', c_void_p), ('diag', c_void_p),
        ('norm_ws', c_void_p), ('norm_ws_bytes', c_size_t), ('skipped', c_void_p), ('prop_ws', c_void_p), ('prop_ws_floats', c_size_t),
        ('xw', c_void_p), ('op', c_void_p * 2), ('gi', c_void_p), ('gh', c_void_p),
        ('out', c_void_p * 2),
    ]  # fmt: skip


SIGNATURES['tgmx_gcn_workspace_bytes'] = (c_size_t, [c_int64, c_int64])
SIGNATURES['tgmx_gcn_norm_csr'] = (c_int32, [_P, _P, c_int32, _P, c_int64, c_int64, ctypes.c_float, c_int32, _P, _P, _P, _P, _P, c_size_t, _P, _P])
SIGNATURES['tgmx_gcn_propagate'] = (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, c_int64, _P, c_int32, _P, c_int64, ctypes.c_float, _P, _P, c_int64, _P, c_int64, c_int64, _P, c_size_t, _P])
SIGNATURES['tgmx_roland_forward'] = (c_int32, [ctypes.POINTER(RolandFwd), _P])


_CSR = [('indptr', c_void_p), ('cols', c_void_p), ('vals', c_void_p), ('diag', c_void_p)]
_CSR_T = [('indptr_t', c_void_p), ('cols_t', c_void_p), ('vals_t', c_void_p)]


class GcnConvBwd(ctypes.Structure):
    """tgmx_gcn_conv_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('N', c_int64), ('in_ch', c_int32), ('C', c_int32),
        ('x', c_void_p), ('ldx', c_int64), ('WT', c_void_p), ('ldwt', c_int64), ('dout', c_void_p), ('lddo', c_int64),
        *_CSR, ('nnz', c_int64), *_CSR_T,
        ('d_W', c_void_p), ('d_b', c_void_p), ('d_x', c_void_p),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


class TgcnCsrFwd(ctypes.Structure):
    """tgmx_tgcn_csr_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('x', c_void_p), ('ldx', c_int64), ('N', c_int64), ('in_ch', c_int32), ('C', c_int32),
        ('src', c_void_p), ('dst', c_void_p), ('edge_w', c_void_p), ('E', c_int64), ('idx64', c_int32), ('fill', ctypes.c_float),
        ('add_self_loops', c_int32), ('csr_built', c_int32), ('save', c_int32),
        ('W3', c_void_p), ('ldw3', c_int64), ('b3', c_void_p),
        ('lin_w', c_void_p * 3), ('lin_b', c_void_p * 3),
        ('H', c_void_p),
        *_CSR,
        ('norm_ws', c_void_p), ('norm_ws_bytes', c_size_t), ('skipped', c_void_p), ('prop_ws', c_void_p), ('prop_ws_floats', c_size_t),
        ('xw', c_void_p), ('G', c_void_p), ('cat', c_void_p * 3), ('pre', c_void_p * 3),
        ('out', c_void_p),
    ]  # fmt: skip


class TgcnCsrBwd(ctypes.Structure):
    """tgmx_tgcn_csr_bwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('N', c_int64), ('in_ch', c_int32), ('C', c_int32),
        ('x', c_void_p), ('ldx', c_int64), ('H', c_void_p),
        ('W3T', c_void_p), ('ldw3t', c_int64), ('lin_wT', c_void_p * 3),
        ('cat', c_void_p * 3), ('pre', c_void_p * 3),
        ('dout', c_void_p),
        *_CSR, ('nnz', c_int64), *_CSR_T,
        ('d_W3', c_void_p), ('d_b3', c_void_p), ('d_lw', c_void_p * 3), ('d_lb', c_void_p * 3), ('d_x', c_void_p), ('d_H', c_void_p),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


SIGNATURES['tgmx_csr_transpose_workspace_bytes'] = (c_size_t, [c_int64, c_int64])
SIGNATURES['tgmx_csr_transpose'] = (c_int32, [_P, _P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_gcn_conv_backward_csr_workspace_bytes'] = (c_size_t, [ctypes.POINTER(GcnConvBwd)])
SIGNATURES['tgmx_gcn_conv_backward_csr'] = (c_int32, [ctypes.POINTER(GcnConvBwd), _P])
SIGNATURES['tgmx_tgcn_forward_csr'] = (c_int32, [ctypes.POINTER(TgcnCsrFwd), _P])
SIGNATURES['tgmx_tgcn_gather_left'] = (c_int32, [_P, _P, _P, c_int32, c_int64, _P, _P])
SIGNATURES['tgmx_tgcn_backward_csr_workspace_bytes'] = (c_size_t, [ctypes.POINTER(TgcnCsrBwd)])
SIGNATURES['tgmx_tgcn_backward_csr'] = (c_int32, [ctypes.POINTER(TgcnCsrBwd), _P])

class HistNeg(ctypes.Structure):
    """tgmx_histneg_t (include/tgm_amd.h)."""

    _fields_ = [
        ('cnt', c_void_p), ('tail', c_void_p), ('num_nodes', c_int64),
        ('pool', c_void_p), ('pool_cap', c_int64),
        ('state', c_void_p),
        ('memory', c_void_p), ('mem_cap', c_int64), ('count', c_int64),
        ('seed', ctypes.c_uint64), ('call', ctypes.c_uint64),
    ]  # fmt: skip


SIGNATURES['tgmx_histneg_workspace_bytes'] = (c_size_t, [c_int64, c_int64])
SIGNATURES['tgmx_histneg_step'] = (c_int32, [ctypes.POINTER(HistNeg), _P, c_int32, _P, c_int32, _P, c_int64, _P, _P, _P, _P, c_size_t, _P])


class TgbNeg(ctypes.Structure):
    """tgmx_tgbneg_t (include/tgm_amd.h)."""

    _fields_ = [
        ('keys', c_void_p), ('indptr', c_void_p), ('rowlen', c_void_p), ('pool', c_void_p),
        ('P', c_int64), ('pool_ints', c_int64),
        ('slots', c_void_p), ('capacity', c_int64),
        ('bitmap', c_void_p), ('bitmap_words', c_int64),
        ('first_missing', c_void_p), ('block_counts', c_void_p), ('num_blocks', c_int64),
        ('qpad', c_int32), ('field', c_int32 * 4), ('reserved', c_int32),
    ]  # fmt: skip


TGBNEG_DUPLICATE, TGBNEG_FULL = 1, 2  # TGMX_TGBNEG_*
SIGNATURES['tgmx_tgbneg_limit'] = (c_int64, [c_int32])
SIGNATURES['tgmx_tgbneg_build'] = (c_int32, [ctypes.POINTER(TgbNeg), _P, _P])
SIGNATURES['tgmx_tgbneg_query'] = (c_int32, [ctypes.POINTER(TgbNeg), _P, c_int32, _P, c_int32, _P, c_int32, _P, c_int32, c_int64, _P, _P, c_int64, _P, _P])
SIGNATURES['tgmx_tgbneg_unique'] = (c_int32, [ctypes.POINTER(TgbNeg), _P, c_int64, _P, c_int32, _P, c_int64, _P, _P])


DECODER_MAX_LAYERS = 8  # TGMX_DECODER_MAX_LAYERS
DECODER_MAX_TAIL = 16  # widest last layer the row-dot kernels take
DECODER_MAX_H = 512  # widest half row of tgmx_decoder_score
DECODER_ROW_MLP_MAX = 4096  # widest layer of tgmx_decoder_row_mlp
DECODER_FORM = {'rows': 0, 'pair': 1, 'table': 2}  # TGMX_DECODER_*
DECODER_POOL = {None: 0, 'mean': 1, 'sum': 2}  # TGMX_DECODER_POOL_*


class DecoderLayer(ctypes.Structure):
    """tgmx_decoder_layer_t (include/tgm_amd.h)."""

    _fields_ = [('w', c_void_p), ('b', c_void_p), ('in_', c_int32), ('out', c_int32)]


class DecoderFwd(ctypes.Structure):
    """tgmx_decoder_fwd_t (include/tgm_amd.h)."""

    _fields_ = [
        ('form', c_int32), ('merge_act', c_int32), ('pool', c_int32), ('num_layers', c_int32),
        ('a1', c_void_p), ('lda1', c_int64), ('n1', c_int64), ('a2', c_void_p), ('lda2', c_int64), ('n2', c_int64),
        ('ia', c_void_p), ('ib', c_void_p), ('neg', c_void_p), ('off', c_void_p), ('idx64', c_int32), ('reserved_', c_int32),
        ('M', c_int64), ('max_candidates', c_int64), ('B', c_int64), ('R', c_int64),
        ('wa', c_void_p), ('ldwa', c_int64), ('wb', c_void_p), ('ldwb', c_int64), ('mbias', c_void_p), ('D', c_int32), ('H', c_int32),
        ('layers', DecoderLayer * DECODER_MAX_LAYERS),
        ('P', c_void_p), ('h', c_void_p * 2), ('pooled', c_void_p), ('pool_ws', c_void_p), ('pool_ws_floats', c_size_t), ('bad', c_void_p),
        ('out', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_decoder_pair_gemm'] = (c_int32, [_P, c_int64, c_int64, _P, _P, c_int64, c_int64, _P, _P, c_int64, c_int32, _P, c_int64, c_int32, _P, c_int32,
                                                  _P, c_int64, c_int64, c_int32, _P, _P])
SIGNATURES['tgmx_decoder_score'] = (c_int32, [_P, c_int64, c_int64, c_int32, _P, _P, _P, c_int32, _P, c_int64, c_int64, c_int64, c_int32, _P, _P, c_int32,
                                              _P, c_int64, _P, _P])
SIGNATURES['tgmx_decoder_tail'] = (c_int32, [_P, c_int64, c_int64, c_int32, _P, _P, c_int32, _P, _P])
SIGNATURES['tgmx_pool_rows_scratch_floats'] = (c_size_t, [c_int64, c_int32])
SIGNATURES['tgmx_pool_rows'] = (c_int32, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_size_t, _P, _P])
SIGNATURES['tgmx_decoder_row_mlp'] = (c_int32, [_P, ctypes.POINTER(DecoderLayer), c_int32, _P, _P])
SIGNATURES['tgmx_decoder_forward'] = (c_int32, [ctypes.POINTER(DecoderFwd), _P])


class DropJob(ctypes.Structure):
    """tgmx_drop_job_t (include/tgm_amd.h)."""

    _fields_ = [('src', c_void_p), ('dst', c_void_p), ('lds', c_int64), ('ldd', c_int64), ('C', c_int32), ('reserved_', c_int32)]


class DecoderTrain(ctypes.Structure):
    """tgmx_decoder_train_t (include/tgm_amd.h)."""

    _fields_ = [
        ('fwd', DecoderFwd), ('act', c_void_p * DECODER_MAX_LAYERS),
        ('dout', c_void_p), ('lddout', c_int64),
        ('d_a1', c_void_p), ('d_a2', c_void_p), ('d_wa', c_void_p), ('ld_dwa', c_int64), ('d_wb', c_void_p), ('ld_dwb', c_int64),
        ('d_mbias', c_void_p), ('d_mbias2', c_void_p),
        ('d_w', c_void_p * DECODER_MAX_LAYERS), ('d_b', c_void_p * DECODER_MAX_LAYERS),
        ('workspace', c_void_p), ('workspace_bytes', c_size_t),
    ]  # fmt: skip


SIGNATURES['tgmx_decoder_tail_bwd_workspace_floats'] = (c_size_t, [c_int64, c_int32, c_int32])
SIGNATURES['tgmx_decoder_tail_bwd'] = (c_int32, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P, c_int32, c_int32, _P, c_int64, _P, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_decoder_scatter_workspace_bytes'] = (c_size_t, [c_int64, c_int64, c_int32])
SIGNATURES['tgmx_decoder_scatter'] = (c_int32, [_P, c_int64, c_int64, c_int32, _P, _P, c_int32, c_int64, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_decoder_drop_rows'] = (c_int32, [_P, _P, c_int32, c_int64, c_int64, ctypes.POINTER(DropJob), c_int32, _P])
SIGNATURES['tgmx_decoder_forward_save'] = (c_int32, [ctypes.POINTER(DecoderTrain), _P])
SIGNATURES['tgmx_decoder_backward_workspace_bytes'] = (c_size_t, [ctypes.POINTER(DecoderTrain)])
SIGNATURES['tgmx_decoder_backward'] = (c_int32, [ctypes.POINTER(DecoderTrain), _P])

AN_BAD_ID, AN_TABLE_FULL, AN_BAD_TIME = 1, 2, 4  # TGMX_AN_*


class AnBatch(ctypes.Structure):
    """tgmx_an_batch_t (include/tgm_amd.h)."""

    _fields_ = [
        ('src', c_void_p), ('dst', c_void_p), ('E', c_int64), ('src_is64', c_int32), ('dst_is64', c_int32),
        ('edge_time', c_void_p), ('Et', c_int64), ('edge_time_is64', c_int32), ('reserved0_', c_int32),
        ('nids', c_void_p), ('Nn', c_int64), ('nids_is64', c_int32), ('reserved1_', c_int32),
        ('node_time', c_void_p), ('Nt', c_int64), ('node_time_is64', c_int32), ('reserved2_', c_int32),
    ]  # fmt: skip


class NodeAnalytics(ctypes.Structure):
    """tgmx_node_analytics_t (include/tgm_amd.h)."""

    _fields_ = [
        ('slot_of', c_void_p), ('num_nodes', c_int64), ('T', c_int64),
        ('first_seen', c_void_p), ('last_seen', c_void_p), ('appearances', c_void_p),
        ('edges', c_void_p), ('edges_cap', c_int64), ('nbrs', c_void_p), ('nbrs_cap', c_int64),
        ('times', c_void_p), ('times_cap', c_int64), ('apps', c_void_p), ('apps_cap', c_int64),
        ('counters', c_void_p),
        ('degree', c_void_p), ('new_nbrs', c_void_p), ('present', c_void_p), ('stamp', c_void_p), ('scalars', c_void_p),
    ]  # fmt: skip


SIGNATURES['tgmx_batch_analytics_workspace_bytes'] = (c_size_t, [c_int64, c_int64, c_int64, c_int64])
SIGNATURES['tgmx_batch_analytics'] = (c_int32, [ctypes.POINTER(AnBatch), c_int32, _P, _P, c_size_t, _P])
SIGNATURES['tgmx_seen_nodes_step'] = (c_int32, [_P, c_int64, _P, c_int32, _P, c_int32, c_int64, _P, c_int32, c_int64, _P, _P, _P, _P])
SIGNATURES['tgmx_node_analytics_step'] = (c_int32, [ctypes.POINTER(NodeAnalytics), ctypes.POINTER(AnBatch), c_int64, _P, _P])
SIGNATURES['tgmx_node_analytics_rehash'] = (c_int32, [_P, c_int64, _P, c_int64, _P, _P])

_lib: Optional[ctypes.CDLL] = None


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """dlopen the kernel library and type every exported entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeLibraryError(
            f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(or `make -C tgm_amd/csrc`). tgm_amd has no CPU fallback.'
        )
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f'failed to load {path}: {e}') from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f'{path} does not export {name}; rebuild it') from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def require_device(t: torch.Tensor, what: str) -> None:
    if t.device.type != 'cuda':
        raise NativeLibraryError(
            f'{what} lives on {t.device}; tgm_amd kernels run only on a ROCm device (there is no CPU fallback). '
            "Create the DGraph with device='cuda'."
        )


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().tgmx_last_error()
        raise RuntimeError(f'{what} failed (rc={rc}): {msg.decode() if msg else "?"}')


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cuda_get_device = getattr(torch._C, '_cuda_getDevice', None)


def stream_ptr(device_index: Optional[int] = None) -> int:
    """hipStream_t of torch's current stream (on ``device_index``, default: the current device).  Goes straight to the C
    accessor: ``torch.cuda.current_stream()`` builds a Stream object through several Python layers (~8 us per call)."""
    if _raw_stream is not None:
        if device_index is None:
            device_index = _cuda_get_device() if _cuda_get_device is not None else torch.cuda.current_device()
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


class KernelTimer:
    """A (start, stop) pair of HIP events recorded by the library right around one kernel launch."""

    def __init__(self) -> None:
        lib = load()
        a, b = c_void_p(), c_void_p()
        check(lib.tgmx_event_create(ctypes.byref(a)), 'tgmx_event_create')
        check(lib.tgmx_event_create(ctypes.byref(b)), 'tgmx_event_create')
        self.start, self.stop = a.value, b.value

    def elapsed_ms(self) -> float:
        ms = ctypes.c_float()
        check(load().tgmx_event_elapsed_ms(self.start, self.stop, ctypes.byref(ms)), 'tgmx_event_elapsed_ms')
        return float(ms.value)

    def __del__(self) -> None:
        try:
            lib = load()
            lib.tgmx_event_destroy(self.start)
            lib.tgmx_event_destroy(self.stop)
        except Exception:
            pass
