"""``DyGFormer`` with its ``NeighborCooccurrenceEncoder`` and ``TransformerEncoder`` (tgm/nn/encoder/dygformer.py; same constructor
arguments, defaults, errors and ``state_dict`` layout: ``time_encoder.w.*``, ``co_occurrence_encoder.neighbor_co_occurrence_encoder.{0,2}.*``,
``projection_layer.{node,edge,time,neighbor_co_occurrence}.*``, ``transformers.{i}.{multi_head_attention,linear_layers,norm_layers}.*``,
``output_layer.*`` -- a checkpoint of the reference's example loads with ``strict=True``).

``forward(node_x, edge_index, edge_time, neighbours, neighbours_time, neighbours_edge_feat) -> (src_emb, dst_emb)``: rows ``[:P]`` of the
three neighbour tensors belong to ``edge_index[0]``, rows ``[P:2P]`` to ``edge_index[1]``.  Every seed is slot 0 of its own sequence (time
gap 0, zero edge features), so a sequence has L = 1 + k slots and L must equal ``max_input_sequence_length``.  Four channels per slot --
node features, edge features, Time2Vec of the time gap, neighbour co-occurrence encoding -- are cut into patches of ``patch_size`` slots,
projected to ``channel_embedding_dim`` each and stacked; the ``2 L / patch_size`` tokens of a (source, destination) pair go through the
transformer layers together; each side's tokens are averaged and passed through ``output_layer``.

``encode_pairs(node_x, src, dst, edge_time, nbr_nids, nbr_edge_time, nbr_edge_x, src_rows, dst_rows)`` is the same computation reading
hop 0 of the sampler's batch in place: ``src_rows`` / ``dst_rows`` [P] index its rows (what ``batch.seed_node_nbr_mask[...]`` holds), so
the gathered copies of ``nbr_edge_x`` & co. that ``forward`` is handed are never made.  ``forward`` is ``encode_pairs`` with identity rows.

Inference (no gradient needed, no active dropout) is ONE native call, ``tgmx_dygformer_forward``: the launches of ``_forward_launches``
in the same order (identical results; ``TGMX_DYGFORMER_PY`` selects the launch-by-launch twin), the argument block cached against the
parameters' versions, the scratch kept between batches.

Training (gradients enabled with a parameter that wants one, dropout included) is native too (``_dygformer_train.py``): the forward is the
same call in its saving form, ``tgmx_dygformer_forward_train`` -- with dropout off (``.train()`` at dropout 0, or ``.eval()``) it returns
the inference bits -- and ``loss.backward()`` is ONE call, ``tgmx_dygformer_backward``: the attention backward recomputes the
probabilities in LDS (``tgmx_mha_small_backward``), the dense contractions run on the exact-fp32 GEMMs, every parameter gets its gradient
(time encoder and co-occurrence encoder included; a frozen one skips its tail).  The four dropout sites of a layer (attention
probabilities, attention output, FFN hidden, FFN output) are counter-based masks regenerated in the backward.  ``TransformerEncoder`` alone
trains through the same layer kernels and also returns the gradient of its input.  ``TGMX_DYGFORMER_BWD`` = ``native`` (default), ``py``
(the backward's launches one ctypes call each, same bits) or ``torch``.

The composed path -- the same arithmetic from torch ops on the device under autograd, with the same parameters -- remains for what is
outside the training envelope: ``TGMX_DYGFORMER_BWD=torch``, a gradient wanted for ``node_x`` or the edge features, autocast, parameters
that are not contiguous float32 on one device, a custom time encoder, a layer whose ``nn.Dropout`` or attention ``dropout`` differs from
the model's ``dropout``, a shape outside ``tgmx_mha_small_train_supported`` (the attention backward keeps Q, K, V, dO and two T x T tiles
in LDS: 2 x 32 patches at head dimension 100 fit, 64 tokens at head dimension 128 and 128 tokens at head dimension 32 do not), and
train-mode dropout with gradients disabled.  ``NeighborCooccurrenceEncoder.forward`` alone stays composed under gradients.  A shape outside
the native inference envelope (more than 128 tokens per pair, a head dimension above 128, more than 2048 slots per sequence, more than 8
layers) also takes the composed path on the device, and so does a device that cannot give the attention kernels their LDS
(``TGMX_E_UNSUPPORTED``).  CPU tensors raise ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .. import _native
from ..constants import PADDED_NODE_ID
from . import _dygformer_train as _train
from ._fwd_plumbing import Unsupported, cached_block, carve_scratch, check_supported, i32, i64, needs_torch, pair_inputs, up4, weight_keeper
from ._paramver import TransientCaches
from .time_encoding import Time2Vec


def _cooccurrence(enc: Optional['NeighborCooccurrenceEncoder'], src: Tensor, dst: Tensor, nids: Tensor, src_rows: Optional[Tensor],
                  dst_rows: Optional[Tensor], counts: Optional[Tensor], feat: Optional[Tensor], ldf: int, table: Optional[Tensor]) -> None:  # fmt: skip
    """``tgmx_dygformer_cooccurrence`` (counts [2 P L, 2] int32 and / or encoded features [2 P L, ldf], pair-major sequence order)."""
    w = [None] * 4 if enc is None else [enc.neighbor_co_occurrence_encoder[i].weight for i in (0, 2)] + [enc.neighbor_co_occurrence_encoder[i].bias for i in (0, 2)]
    p = _native.ptr
    _native.check(
        _native.load().tgmx_dygformer_cooccurrence(src.data_ptr(), dst.data_ptr(), src.numel(), p(nids), nids.shape[0], nids.shape[1], p(src_rows),
                                                   p(dst_rows), p(w[0]), p(w[2]), p(w[1]), p(w[3]), 0 if enc is None else enc.feat_dim, p(table),
                                                   p(counts), p(feat), ldf, _native.stream_ptr()),
        'tgmx_dygformer_cooccurrence',
    )  # fmt: skip


class NeighborCooccurrenceEncoder(nn.Module):
    r"""Neighbour co-occurrence encoding (https://arxiv.org/abs/2303.13047, Section 4.1): slot j of a sequence is described by how often
    its node id occurs in its own sequence and in the other sequence of the pair; each count goes through Linear(1, d) -> ReLU -> Linear(d, d)
    and the two results are summed.  Padded slots count as 0 (and still go through the encoder)."""

    def __init__(self, feat_dim: int, device: str) -> None:
        super().__init__()
        self.feat_dim, self.device = feat_dim, device
        self.neighbor_co_occurrence_encoder = nn.Sequential(nn.Linear(1, feat_dim), nn.ReLU(), nn.Linear(feat_dim, feat_dim)).to(device)

    def _split(self, src_ids: Tensor, dst_ids: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        _native.require_device(src_ids, 'src_neighbour_nodes_ids')
        _native.require_device(dst_ids, 'dst_neighbour_nodes_ids')
        if src_ids.dim() != 2 or src_ids.shape != dst_ids.shape or src_ids.shape[1] < 1:
            raise ValueError(f'expected two [P, L] id matrices of one shape, got {list(src_ids.shape)} and {list(dst_ids.shape)}')
        if src_ids.shape[1] > _native.DYGFORMER_MAX_SEQ:
            raise NotImplementedError(f'tgm_amd NeighborCooccurrenceEncoder: at most {_native.DYGFORMER_MAX_SEQ} slots per sequence')
        s, d = i32(src_ids), i32(dst_ids)
        return s[:, 0].contiguous(), d[:, 0].contiguous(), torch.cat([s[:, 1:], d[:, 1:]], dim=0).contiguous()

    def _count_nodes_freq(self, src_nbrs: Tensor, dst_nbrs: Tensor) -> Tuple[Tensor, Tensor]:
        """([P, L, 2], [P, L, 2]) float: (occurrences in the own sequence, occurrences in the other one), 0 for padded slots."""
        src, dst, nids = self._split(src_nbrs, dst_nbrs)
        P, L = src_nbrs.shape
        counts = torch.empty((P, 2, L, 2), dtype=torch.int32, device=src.device)
        if P:
            _cooccurrence(None, src, dst, nids, None, None, counts, None, 0, None)
        return counts[:, 0].float(), counts[:, 1].float()

    def forward(self, src_neighbour_nodes_ids: Tensor, dst_neighbour_nodes_ids: Tensor) -> Tuple[Tensor, Tensor]:
        src, dst, nids = self._split(src_neighbour_nodes_ids, dst_neighbour_nodes_ids)
        P, L = src_neighbour_nodes_ids.shape
        if needs_torch(self, 0.0):
            return self._torch_forward(i64(src_neighbour_nodes_ids), i64(dst_neighbour_nodes_ids))  # training: torch ops (not native)
        C = self.feat_dim
        feat = torch.empty((P, 2, L, C), dtype=torch.float32, device=src.device)
        if P:
            table = torch.empty((L + 1, C), dtype=torch.float32, device=src.device)
            _cooccurrence(self, src, dst, nids, None, None, None, feat, C, table)
        return feat[:, 0], feat[:, 1]

    def _torch_forward(self, s: Tensor, d: Tensor) -> Tuple[Tensor, Tensor]:
        """The same from torch ops (autograd-capable; not native): s, d [P, L] int64."""
        own = lambda a: (a.unsqueeze(1) == a.unsqueeze(2)).sum(dim=2)
        other = lambda a, b: (a.unsqueeze(2) == b.unsqueeze(1)).sum(dim=2)
        out = []
        for a, b in ((s, d), (d, s)):
            cnt = torch.stack([own(a), other(a, b)], dim=2).float() * (a != PADDED_NODE_ID).unsqueeze(-1)
            out.append(self.neighbor_co_occurrence_encoder(cnt.unsqueeze(-1)).sum(dim=2))
        return out[0], out[1]


def _layer_block(t: 'TransformerEncoder', f32: Callable[..., int]) -> '_native.DyGFormerLayer':
    mha, ln, lin = t.multi_head_attention, t.norm_layers, t.linear_layers
    if mha.in_proj_weight is None or mha.in_proj_bias is None or mha.bias_k is not None or mha.batch_first:
        raise NotImplementedError('tgm_amd TransformerEncoder: the native layer needs the packed in-projection with bias')
    ly = _native.DyGFormerLayer()
    names = ('ln0_g', 'ln0_b', 'in_w', 'in_b', 'out_w', 'out_b', 'ln1_g', 'ln1_b', 'w1', 'b1', 'w2', 'b2')
    tensors = (ln[0].weight, ln[0].bias, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, ln[1].weight, ln[1].bias,
               lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias)  # fmt: skip
    for n, p in zip(names, tensors):
        setattr(ly, n, f32(p, n))
    return ly


def _native_layer(t: 'TransformerEncoder', B: int, T: int, x: Tensor, y: Tensor, x1: Tensor, att: Tensor, ldx: int, qkv: Tensor, ldq: int, h: Tensor,
                  ldh: int) -> None:  # fmt: skip
    """``tgmx_dygformer_layer`` on x [B T, ldx], in place."""
    keep, f32 = weight_keeper()  # (keep: the converted weights outlive the launch)
    ly = _layer_block(t, f32)
    check_supported(
        _native.load().tgmx_dygformer_layer(ctypes.byref(ly), B, T, t.num_heads, t.attention_dim, float(t.norm_layers[0].eps), x.data_ptr(), y.data_ptr(),
                                            x1.data_ptr(), att.data_ptr(), ldx, qkv.data_ptr(), ldq, h.data_ptr(), ldh, _native.stream_ptr()),
        'tgmx_dygformer_layer',
    )  # fmt: skip


def _mha_in_envelope(T: int, D: int, H: int) -> bool:
    return T <= _native.MHA_SMALL_MAX_TOKENS and D // H <= _native.MHA_SMALL_MAX_HEAD_DIM


class TransformerEncoder(nn.Module):
    r"""One DyGFormer transformer layer on [B, T, d]: ``x1 = x + MHA(LN0(x))`` (self-attention over the T tokens of each batch entry, no
    mask; the residual takes the un-normalised input), ``out = x1 + Linear(GELU(Linear_4x(LN1(x1))))``.  Inference is native
    (``tgmx_dygformer_layer``: LayerNorm, exact-fp32 MFMA GEMMs, ``tgmx_mha_small``) for T <= 128 and head dimension <= 128, and so is
    training inside ``_dygformer_train.layer_in_envelope`` (``tgmx_dygformer_layer_train`` / ``tgmx_dygformer_layer_backward``, dropout
    included); otherwise the same arithmetic composed from torch ops on the device (not native)."""

    def __init__(self, attention_dim: int, num_heads: int, dropout: float = 0.1) -> None:
        super().__init__()
        self.attention_dim, self.num_heads, self.dropout_rate = attention_dim, num_heads, dropout
        self.multi_head_attention = nn.MultiheadAttention(embed_dim=attention_dim, num_heads=num_heads, dropout=dropout)
        self.dropout = nn.Dropout(dropout)
        self.linear_layers = nn.ModuleList([nn.Linear(attention_dim, 4 * attention_dim), nn.Linear(4 * attention_dim, attention_dim)])
        self.norm_layers = nn.ModuleList([nn.LayerNorm(attention_dim), nn.LayerNorm(attention_dim)])

    def _torch_forward(self, inputs: Tensor) -> Tensor:
        h = self.norm_layers[0](inputs).transpose(0, 1)
        x1 = inputs + self.dropout(self.multi_head_attention(h, h, h, need_weights=False)[0].transpose(0, 1))
        h = self.linear_layers[1](self.dropout(F.gelu(self.linear_layers[0](self.norm_layers[1](x1)))))
        return x1 + self.dropout(h)

    def _check_native(self) -> None:
        if self.norm_layers[0].eps != self.norm_layers[1].eps:
            raise NotImplementedError('tgm_amd TransformerEncoder: the native layer takes one LayerNorm eps for both norms')

    def forward(self, inputs: Tensor) -> Tensor:
        _native.require_device(inputs, 'TransformerEncoder input')
        if inputs.dim() != 3 or inputs.shape[2] != self.attention_dim:
            raise ValueError(f'TransformerEncoder expects [B, T, {self.attention_dim}], got {list(inputs.shape)}')
        B, T, D = inputs.shape
        if _train.layer_in_envelope(self, inputs):
            try:
                return _train.apply_layer(self, inputs)
            except Unsupported:  # the device cannot give the attention kernels their LDS: compose
                return self._torch_forward(inputs)
        if needs_torch(self, self.dropout_rate, inputs) or not _mha_in_envelope(T, D, self.num_heads) or B * T == 0:
            return self._torch_forward(inputs)
        self._check_native()
        ldx = up4(D)
        f32 = dict(dtype=torch.float32, device=inputs.device)
        x = torch.zeros((B * T, ldx), **f32)
        x[:, :D] = inputs.reshape(B * T, D)
        y, x1, att = (torch.empty((B * T, ldx), **f32) for _ in range(3))
        qkv, h = torch.empty((B * T, up4(3 * D)), **f32), torch.empty((B * T, 4 * D), **f32)
        try:
            _native_layer(self, B, T, x, y, x1, att, ldx, qkv, up4(3 * D), h, 4 * D)
        except Unsupported:  # the device cannot give tgmx_mha_small its LDS: compose
            return self._torch_forward(inputs)
        return x[:, :D].reshape(B, T, D)


class DyGFormer(TransientCaches, nn.Module):
    r"""DyGFormer (https://arxiv.org/abs/2303.13047); see the module docstring for the interface and for what runs natively."""

    CHANNELS = ('node', 'edge', 'time', 'neighbor_co_occurrence')

    def __init__(self, node_feat_dim: int, edge_x_dim: int, time_feat_dim: int, channel_embedding_dim: int, output_dim: int = 172,
                 patch_size: int = 1, num_layers: int = 2, num_heads: int = 2, dropout: float = 0.1, max_input_sequence_length: int = 512,
                 num_channels: int = 4, time_encoder: Callable[..., nn.Module] = Time2Vec, device: str = 'cpu') -> None:  # fmt: skip
        super().__init__()
        if max_input_sequence_length % patch_size != 0:
            raise ValueError('Max sequence length must be a multiple of path size')
        if num_channels != 4:
            raise NotImplementedError(f'DyGFormer stacks four channels (node, edge, time, co-occurrence); num_channels={num_channels} has no meaning')
        self.node_feat_dim, self.edge_x_dim, self.time_feat_dim = node_feat_dim, edge_x_dim, time_feat_dim
        self.channel_embedding_dim, self.patch_size, self.max_input_sequence_length = channel_embedding_dim, patch_size, max_input_sequence_length
        self.neighbor_co_occurrence_feat_dim = channel_embedding_dim
        self.device, self.num_channels, self.num_patches = device, num_channels, max_input_sequence_length // patch_size
        self.output_dim, self.num_layers, self.num_heads, self.dropout = output_dim, num_layers, num_heads, dropout
        self.time_encoder = time_encoder(time_feat_dim)
        self.co_occurrence_encoder = NeighborCooccurrenceEncoder(feat_dim=channel_embedding_dim, device=device)
        dims = (node_feat_dim, edge_x_dim, time_feat_dim, channel_embedding_dim)
        self.projection_layer = nn.ModuleDict({n: nn.Linear(patch_size * d, channel_embedding_dim) for n, d in zip(self.CHANNELS, dims)}).to(device)
        self.transformers = nn.ModuleList(
            [TransformerEncoder(attention_dim=num_channels * channel_embedding_dim, num_heads=num_heads, dropout=dropout) for _ in range(num_layers)]
        ).to(device)
        self.output_layer = nn.Linear(num_channels * channel_embedding_dim, output_dim).to(device)

    # -- inputs ------------------------------------------------------------------------------------------------------------------------
    def _check_slots(self, k: int) -> None:
        if 1 + k != self.max_input_sequence_length:
            raise ValueError(f'a sequence is the seed plus its k = {k} sampled neighbours: L = {1 + k} slots, which must equal '
                             f'max_input_sequence_length = {self.max_input_sequence_length} (sample max_input_sequence_length - 1 neighbours)')

    def _inputs(self, *tensors) -> dict:
        """(node_x, src, dst, edge_time, nids, nbr_t, nbr_x, src_rows, dst_rows), checked and converted."""
        a = pair_inputs(*tensors, self.node_feat_dim, self.edge_x_dim, self._check_slots, 'P')
        return dict(a, P=a['src'].numel(), L=1 + a['nids'].shape[1])

    def forward(self, node_x: Tensor, edge_index: Tensor, edge_time: Tensor, neighbours: Tensor, neighbours_time: Tensor,
                neighbours_edge_feat: Tensor) -> Tuple[Tensor, Tensor]:  # fmt: skip
        return self._run(self._inputs(node_x, edge_index[0], edge_index[1], edge_time, neighbours, neighbours_time, neighbours_edge_feat, None, None))

    def encode_pairs(self, node_x: Tensor, src: Tensor, dst: Tensor, edge_time: Tensor, nbr_nids: Tensor, nbr_edge_time: Tensor, nbr_edge_x: Tensor,
                     src_rows: Tensor, dst_rows: Tensor) -> Tuple[Tensor, Tensor]:  # fmt: skip
        """``forward`` on ``nbr_*[cat(src_rows, dst_rows)]`` without making those copies (same results, bit for bit)."""
        return self._run(self._inputs(node_x, src, dst, edge_time, nbr_nids, nbr_edge_time, nbr_edge_x, src_rows, dst_rows))

    def _native_ok(self, L: int) -> bool:
        D = self.num_channels * self.channel_embedding_dim
        return (L <= _native.DYGFORMER_MAX_SEQ and self.num_layers <= _native.DYGFORMER_MAX_LAYERS and hasattr(self.time_encoder, 'w')
                and _mha_in_envelope(2 * self.num_patches, D, self.num_heads))  # fmt: skip

    def _run(self, a: dict) -> Tuple[Tensor, Tensor]:
        grad_inputs = (a['node_x'], a['nbr_x'])
        if _train.in_envelope(self, a):
            for t in self.transformers:
                t._check_native()
            try:
                return _train.apply(self, a)
            except Unsupported:  # the device cannot give the attention kernels their LDS: compose
                return self._torch_forward(a)
        if needs_torch(self, self.dropout, *grad_inputs) or not self._native_ok(a['L']):
            return self._torch_forward(a)
        for t in self.transformers:
            t._check_native()
        P = a['P']
        out = torch.empty((2 * P, self.output_dim), dtype=torch.float32, device=a['node_x'].device)
        if P:
            try:
                if os.environ.get('TGMX_DYGFORMER_PY') is not None:  # A/B: the same launches composed from Python, one ctypes call each
                    self._forward_launches(a, out)
                else:
                    self._forward_native(a, out)
            except Unsupported:  # the device cannot give tgmx_mha_small its LDS: compose
                return self._torch_forward(a)
        return out[:P], out[P:]

    # -- outside the native envelopes: torch ops under autograd (not native) -------------------------------------------------------------
    def _torch_forward(self, a: dict) -> Tuple[Tensor, Tensor]:
        P, L, k = a['P'], a['L'], a['L'] - 1
        dev = a['node_x'].device
        if a['src_rows'] is None:
            rows = torch.arange(2 * P, device=dev)
        else:
            rows = torch.cat([a['src_rows'], a['dst_rows']]).long()
        seeds = torch.cat([a['src'], a['dst']]).long()
        ids = torch.cat([seeds[:, None], a['nids'][rows].long()], dim=1)  # [2P, L]: sources, then destinations
        valid = (ids != PADDED_NODE_ID).unsqueeze(-1)
        node = a['node_x'][ids.clamp(min=0)] * valid
        edge = torch.cat([a['nbr_x'].new_zeros((2 * P, 1, self.edge_x_dim)), a['nbr_x'][rows]], dim=1)
        t = torch.cat([a['t'], a['t']])
        dt = torch.cat([t.new_zeros((2 * P, 1)), t[:, None] - a['nbr_t'][rows]], dim=1).float().unsqueeze(-1)
        tw = getattr(self.time_encoder, 'w', None)
        time = (torch.cos(F.linear(dt, tw.weight, tw.bias)) if tw is not None else self.time_encoder(dt.squeeze(-1))) * valid
        co_s, co_d = self.co_occurrence_encoder._torch_forward(ids[:P], ids[P:])
        Np, pl = self.num_patches, self.projection_layer
        tok = torch.cat([pl[n](f.reshape(2 * P, Np, -1)) for n, f in zip(self.CHANNELS, (node, edge, time, torch.cat([co_s, co_d], dim=0)))], dim=2)
        z = torch.cat([tok[:P], tok[P:]], dim=1)  # [P, 2 Np, 4 C]: the source's patches first
        for tr in self.transformers:
            z = tr._torch_forward(z)
        return self.output_layer(z[:, :Np].mean(dim=1)), self.output_layer(z[:, Np:].mean(dim=1))

    # -- inference ------------------------------------------------------------------------------------------------------------------------
    def _dims(self) -> dict:
        C = self.channel_embedding_dim
        D = 4 * C
        return dict(ldch=[up4(self.node_feat_dim), up4(self.edge_x_dim), up4(self.time_feat_dim), up4(C)], ldx=up4(D), ldq=up4(3 * D), ldh=4 * D)

    def _scratch(self, P: int, L: int, device) -> List[Tensor]:
        """table, ch[0..3], x, y, x1, att, qkv, h, mean: views into one buffer kept between batches."""
        d = self._dims()
        R = 2 * P * self.num_patches
        sizes = [(L + 1) * self.channel_embedding_dim] + [2 * P * L * ld for ld in d['ldch']] + [R * d['ldx']] * 4
        return carve_scratch(self, sizes + [R * d['ldq'], R * d['ldh'], 2 * P * d['ldx']], device)

    def _weights(self) -> tuple:
        """(argument block with the weights filled in, the tensors it points at), cached against the parameters' versions."""

        def build(f32) -> '_native.DyGFormerFwd':
            blk = _native.DyGFormerFwd()
            tw, co = self.time_encoder.w, self.co_occurrence_encoder.neighbor_co_occurrence_encoder
            blk.tw, blk.tb = f32(tw.weight.reshape(-1)), f32(tw.bias)
            blk.co_w1, blk.co_b1, blk.co_w2, blk.co_b2 = f32(co[0].weight.reshape(-1)), f32(co[0].bias), f32(co[2].weight), f32(co[2].bias)
            C, ps = self.channel_embedding_dim, self.patch_size
            dims = (self.node_feat_dim, self.edge_x_dim, self.time_feat_dim, C)
            for c, (n, dc) in enumerate(zip(self.CHANNELS, dims)):
                w = self.projection_layer[n].weight.detach()
                if dc % 4:  # each slot's columns padded to the channel input's leading dimension (zeros)
                    w = F.pad(w.reshape(C, ps, dc), (0, up4(dc) - dc)).reshape(C, ps * up4(dc))
                blk.proj_w[c], blk.proj_b[c] = f32(w), f32(self.projection_layer[n].bias)
            blk.out_w, blk.out_b = f32(self.output_layer.weight), f32(self.output_layer.bias)
            blk.num_layers = self.num_layers
            eps = float(self.transformers[0].norm_layers[0].eps) if self.num_layers else 1e-5
            blk.eps = eps
            for i, t in enumerate(self.transformers):
                if float(t.norm_layers[0].eps) != eps:
                    raise NotImplementedError('tgm_amd DyGFormer: the native forward takes one LayerNorm eps for every layer')
                blk.layers[i] = _layer_block(t, f32)
            blk.k, blk.dN, blk.dE, blk.dT = self.max_input_sequence_length - 1, self.node_feat_dim, self.edge_x_dim, self.time_feat_dim
            blk.C, blk.patch, blk.heads, blk.E = C, ps, self.num_heads, self.output_dim
            return blk

        return cached_block(self, build)

    def _forward_native(self, a: dict, out: Tensor) -> None:
        blk, _ = self._weights()
        P, L = a['P'], a['L']
        d = self._dims()
        bufs = self._scratch(P, L, out.device)
        blk.node_x, blk.num_nodes = a['node_x'].data_ptr(), a['node_x'].shape[0]
        blk.src, blk.dst, blk.edge_time, blk.P = a['src'].data_ptr(), a['dst'].data_ptr(), a['t'].data_ptr(), P
        blk.nbr_nids, blk.nbr_t, blk.nbr_x, blk.S = a['nids'].data_ptr(), a['nbr_t'].data_ptr(), a['nbr_x'].data_ptr(), a['nids'].shape[0]
        blk.src_rows, blk.dst_rows = _native.ptr(a['src_rows']), _native.ptr(a['dst_rows'])
        blk.table = bufs[0].data_ptr()
        for c in range(4):
            blk.ch[c], blk.ldch[c] = bufs[1 + c].data_ptr(), d['ldch'][c]
        blk.x, blk.y, blk.x1, blk.att, blk.qkv, blk.h, blk.mean = (b.data_ptr() for b in bufs[5:12])
        blk.ldx, blk.ldq, blk.ldh = d['ldx'], d['ldq'], d['ldh']
        blk.out = out.data_ptr()
        check_supported(_native.load().tgmx_dygformer_forward(ctypes.byref(blk), _native.stream_ptr()), 'tgmx_dygformer_forward')

    def _forward_launches(self, a: dict, out: Tensor) -> None:
        """The native forward's launches one ctypes call each (the A/B and test twin of ``_forward_native``)."""
        lib, stream = _native.load(), _native.stream_ptr()
        blk, _ = self._weights()  # the padded projection weights
        P, L, k = a['P'], a['L'], a['L'] - 1
        d = self._dims()
        ldch, ldx, ldq, ldh = d['ldch'], d['ldx'], d['ldq'], d['ldh']
        table, ch0, ch1, ch2, ch3, x, y, x1, att, qkv, h, mean = self._scratch(P, L, out.device)
        C, ps, Np = self.channel_embedding_dim, self.patch_size, self.num_patches
        R = 2 * P * Np
        _cooccurrence(self.co_occurrence_encoder, a['src'], a['dst'], a['nids'], a['src_rows'], a['dst_rows'], None, ch3, ldch[3], table)
        tw = self.time_encoder.w
        p = _native.ptr
        _native.check(
            lib.tgmx_dygformer_prologue(a['node_x'].data_ptr(), a['node_x'].shape[0], self.node_feat_dim, a['src'].data_ptr(), a['dst'].data_ptr(),
                                        a['t'].data_ptr(), P, a['nids'].data_ptr(), a['nbr_t'].data_ptr(), a['nbr_x'].data_ptr(), a['nids'].shape[0], k,
                                        self.edge_x_dim, p(a['src_rows']), p(a['dst_rows']), tw.weight.data_ptr(), tw.bias.data_ptr(), self.time_feat_dim,
                                        ch0.data_ptr(), ldch[0], ch1.data_ptr(), ldch[1], ch2.data_ptr(), ldch[2], stream),
            'tgmx_dygformer_prologue',
        )  # fmt: skip
        for c, (n, buf) in enumerate(zip(self.CHANNELS, (ch0, ch1, ch2, ch3))):
            Kc = ps * ldch[c]
            _native.check(
                lib.tgmx_sgemm_nt_ep(buf.data_ptr(), Kc, blk.proj_w[c], Kc, x.data_ptr() + 4 * c * C, ldx, R, C, Kc, blk.proj_b[c], 0, None, 0, stream),
                'tgmx_sgemm_nt_ep',
            )  # fmt: skip
        for t in self.transformers:
            _native_layer(t, P, 2 * Np, x, y, x1, att, ldx, qkv, ldq, h, ldh)
        ol = self.output_layer
        _native.check(
            lib.tgmx_dygformer_tail(x.data_ptr(), ldx, P, Np, 4 * C, mean.data_ptr(), ldx, ol.weight.data_ptr(), ol.bias.data_ptr(), self.output_dim,
                                    out.data_ptr(), stream),
            'tgmx_dygformer_tail',
        )  # fmt: skip
