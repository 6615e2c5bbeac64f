"""``GraphMixerEncoder`` -- GraphMixer's link + node encoder (the reference keeps it in examples/linkproppred/graphmixer.py; a tgm_amd
extension).  Same constructor arguments and ``state_dict`` layout as the example: ``time_encoder.w.*`` (frozen), ``projection_layer``,
``mlp_mixers.{i}.*``, ``output_layer`` -- a checkpoint trained with the example loads unchanged.

``forward(batch, node_feat)`` -> [3 bs, embed_dim], rows in the order src, dst, neg.  It reads hop 0 of a ``RecencyNeighborHook`` over
the seeds ``edge_src, edge_dst, neg`` and the outputs of ``TimeGapNeighborHook``:

* link encoder: [nbr_edge_x | Time2Vec(seed_time - nbr_edge_time)] -> projection -> MLPMixer layers -> mean over the valid slots
  (``nbr_nids != -1``; padded slots still take part in token mixing with whatever the sampler wrote for them);
* node encoder: mean of ``node_feat`` over the seed's time-gap neighbours (zero when there are none) + ``node_feat[seed]``;
* ``output_layer([link | node])``.

Inference (no gradient needed, no active dropout) is ONE native call, ``tgmx_graphmixer_forward``: the launches of ``_forward_launches``
in the same order (identical results), the argument block cached against the parameters' versions, the scratch kept between batches.
The native envelope is ``tgmx_mixer_token``'s: a seed's tile of ``4 * (K D + (K + Ht) * 128)`` bytes (K = num_tokens, D = edge_dim,
Ht = int(token_dim_expansion * K)) fits 64 KiB of LDS.  Outside it (num_tokens = 64 at edge_dim = 172, say) the call answers
``TGMX_E_UNSUPPORTED`` and inference is the composed torch arithmetic of the training path, under ``torch.no_grad()`` (a
``RuntimeWarning`` says so, once per module).
Training (gradients enabled) is native inside the same kind of envelope (``_graphmixer_train.py``): the forward is the inference call in
its saving form -- the bits of the no-grad output when dropout is off -- and ``loss.backward()`` is ONE native call,
``tgmx_graphmixer_backward``.  The envelope: float32 ``node_feat`` / edge features on the device that ask for no gradient, no autocast,
contiguous float32 parameters, the time encoder frozen as the constructor leaves it, at least one seed, and a seed's tile inside both
token kernels' LDS (the forward's bound above and ``4 * (4 K + 2 Ht) * 33`` bytes for the backward's narrowest pass).  Train mode with dropout > 0 is
native too: counter-based masks (``tgmx_dropout_t``) seeded from ``torch.initial_seed()``, a fresh stream per forward call and site,
regenerated -- not stored -- by the backward.  No gradient reaches ``node_feat``, the edge features or the time encoder.  Everything
else (and ``TGMX_GRAPHMIXER_BWD=torch``) is the reference arithmetic composed from torch ops on the device under autograd, with the
same parameters.  CPU tensors raise ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Any, List

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from ..constants import PADDED_NODE_ID
from . import _graphmixer_train, _ops
from ._fwd_plumbing import Unsupported, cached_block, carve_scratch, check_supported, fill_mixer_layers, i32, i64, needs_torch, up4
from ._paramver import TransientCaches
from .mlp_mixer import MLPMixer, sgemm_ep, token_block, warn_composed
from .time_encoding import Time2Vec


class GraphMixerEncoder(TransientCaches, nn.Module):
    def __init__(self, time_dim: int, embed_dim: int, num_tokens: int, node_dim: int, edge_dim: int, num_layers: int = 2,
                 token_dim_expansion: float = 0.5, channel_dim_expansion: float = 4.0, dropout: float = 0.1) -> None:  # fmt: skip
        super().__init__()
        for name, v in (('time_dim', time_dim), ('embed_dim', embed_dim), ('num_tokens', num_tokens), ('node_dim', node_dim), ('edge_dim', edge_dim)):
            if int(v) != v or v <= 0:
                raise ValueError(f'{name} must be a positive int, got {v}')
        if int(num_layers) != num_layers or not 0 <= num_layers <= _native.MIXER_MAX_LAYERS:
            raise ValueError(f'num_layers must be in [0, {_native.MIXER_MAX_LAYERS}], got {num_layers}')
        if int(channel_dim_expansion * edge_dim) < 1:
            raise ValueError(f'channel_dim_expansion={channel_dim_expansion} leaves no hidden channel for edge_dim={edge_dim}')
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f'dropout must be in [0, 1), got {dropout}')
        self.time_dim, self.embed_dim, self.num_tokens, self.node_dim, self.edge_dim = time_dim, embed_dim, num_tokens, node_dim, edge_dim
        self.num_layers, self.dropout = num_layers, dropout
        self.requires = {'edge_src', 'edge_dst', 'neg', 'nbr_edge_x', 'seed_times', 'nbr_edge_time', 'nbr_nids', 'time_gap_nbr', 'time_gap_lo',
                         'time_gap_cnt'}  # fmt: skip
        # GraphMixer's time encoding is not trainable
        self.time_encoder = Time2Vec(time_dim=time_dim)
        for p in self.time_encoder.parameters():
            p.requires_grad = False
        self.projection_layer = nn.Linear(edge_dim + time_dim, edge_dim)
        self.mlp_mixers = nn.ModuleList([
            MLPMixer(num_tokens=num_tokens, num_channels=edge_dim, token_dim_expansion_factor=token_dim_expansion,
                     channel_dim_expansion_factor=channel_dim_expansion, dropout=dropout)
            for _ in range(num_layers)
        ])  # fmt: skip
        self.output_layer = nn.Linear(in_features=edge_dim + node_dim, out_features=embed_dim)

    # -- inputs ------------------------------------------------------------------------------------------------------------------------
    def _inputs(self, batch: Any, node_feat: Tensor) -> dict:
        _native.require_device(node_feat, 'node_feat')
        for name in ('edge_src', 'edge_dst', 'neg', 'time_gap_nbr', 'time_gap_lo', 'time_gap_cnt'):
            if getattr(batch, name, None) is None:
                raise ValueError(f'GraphMixerEncoder needs batch.{name}')
            _native.require_device(getattr(batch, name), f'batch.{name}')
        ex = _ops._f32c(batch.nbr_edge_x[0], 'nbr_edge_x')
        seeds = [i32(batch.edge_src), i32(batch.edge_dst), i32(batch.neg)]
        S = sum(t.numel() for t in seeds)
        nids = i32(batch.nbr_nids[0])
        if ex.dim() != 3 or tuple(ex.shape) != (S, self.num_tokens, self.edge_dim) or tuple(nids.shape) != (S, self.num_tokens):
            raise ValueError(f'GraphMixerEncoder(num_tokens={self.num_tokens}, edge_dim={self.edge_dim}) expects hop-0 samples of '
                             f'[{S}, {self.num_tokens}(, {self.edge_dim})] over the seeds edge_src | edge_dst | neg, got nbr_edge_x '
                             f'{list(ex.shape)} and nbr_nids {list(nids.shape)}')
        x = _ops._f32c(node_feat, 'node_feat')
        if x.dim() != 2 or x.shape[1] != self.node_dim:
            raise ValueError(f'node_feat must be [num_nodes, {self.node_dim}], got {list(x.shape)}')
        if batch.time_gap_lo.numel() != S or batch.time_gap_cnt.numel() != S:
            raise ValueError('time_gap_lo / time_gap_cnt do not cover the seeds edge_src | edge_dst | neg')
        return dict(ex=ex, seed_t=i64(batch.seed_times[0]), nbr_t=i64(batch.nbr_edge_time[0]), nids=nids, seeds=seeds, S=S, node_x=x,
                    tg_nbr=i32(batch.time_gap_nbr), tg_lo=i32(batch.time_gap_lo), tg_cnt=i32(batch.time_gap_cnt))  # fmt: skip

    def forward(self, batch: Any, node_feat: Tensor) -> Tensor:
        a = self._inputs(batch, node_feat)
        if needs_torch(self, self.dropout, node_feat, a['ex']):
            if _graphmixer_train.in_envelope(self, node_feat, batch.nbr_edge_x[0], a['S']):
                return _graphmixer_train.apply(self, a)  # training: the saving forward, one native call for the backward
            return self._torch_forward(a)
        for m in self.mlp_mixers:
            m._check_native()
        try:
            if os.environ.get('TGMX_GRAPHMIXER_PY') is not None:  # A/B: the same launches composed from Python, one ctypes call each
                return self._forward_launches(a)
            return self._forward_native(a)
        except Unsupported as e:  # a seed's [num_tokens, edge_dim] tile does not fit tgmx_mixer_token's LDS: compose
            warn_composed(self, 'GraphMixerEncoder', str(e))
            with torch.no_grad():
                return self._torch_forward(a)

    # -- training outside the native envelope: torch ops under autograd ------------------------------------------------------------------
    def _torch_forward(self, a: dict) -> Tensor:
        tw = self.time_encoder.w
        dt = (a['seed_t'][:, None] - a['nbr_t']).unsqueeze(-1).float()
        z = self.projection_layer(torch.cat([a['ex'], torch.cos(tw(dt))], dim=-1))
        for m in self.mlp_mixers:
            z = m._torch_forward(z)
        valid = a['nids'] != PADDED_NODE_ID
        z_link = (z * valid.unsqueeze(-1)).sum(dim=1) / valid.sum(dim=1, keepdim=True).clamp(min=1)
        # time-gap mean as a difference of float64 prefix sums over the grouped neighbours: no device -> host read for the run lengths
        x = a['node_x']
        # (the scan runs along the innermost dimension: torch's outer-dimension double scan took ~0.9 ms at cfg 2)
        g = x[a['tg_nbr'].long()].double().t().contiguous()  # [F, 2 W]
        cs = torch.cat([g.new_zeros((g.shape[0], 1)), torch.cumsum(g, dim=1)], dim=1)
        lo, cnt = a['tg_lo'].long(), a['tg_cnt'].long()
        tg = ((cs[:, lo + cnt] - cs[:, lo]) / cnt.clamp(min=1)).t().float()
        z_node = tg + x[torch.cat(a['seeds']).long()]
        return self.output_layer(torch.cat([z_link, z_node], dim=1))

    # -- inference --------------------------------------------------------------------------------------------------------------------
    def _dims(self, S: int) -> dict:
        K, D, T, F_ = self.num_tokens, self.edge_dim, self.time_dim, self.node_dim
        Hc = max(m.channel_feedforward.ffn[0].out_features for m in self.mlp_mixers) if self.num_layers else 4
        return dict(R=S * K, ldx0=up4(D + T), ldz=up4(D), ldh=up4(Hc), ldcat=up4(D + F_))

    def _scratch(self, S: int, device) -> List[Tensor]:
        """x0, z, z1, y, h, cat: views into one buffer kept between batches."""
        d = self._dims(S)
        R = d['R']
        return carve_scratch(self, [R * d['ldx0'], R * d['ldz'], R * d['ldz'], R * d['ldz'], R * d['ldh'], S * d['ldcat']], device)

    def _forward_launches(self, a: dict) -> Tensor:
        """The native forward's launches one ctypes call each (the A/B and test twin of ``_forward_native``)."""
        lib, stream = _native.load(), _native.stream_ptr()
        S, K, D, T = a['S'], self.num_tokens, self.edge_dim, self.time_dim
        d = self._dims(S)
        R, ldx0, ldz, ldh, ldcat = d['R'], d['ldx0'], d['ldz'], d['ldh'], d['ldcat']
        dev = a['ex'].device
        out = torch.empty((S, self.embed_dim), dtype=torch.float32, device=dev)
        if S == 0:
            return out
        x0, z, z1, y, h, cat = self._scratch(S, dev)
        tw = self.time_encoder.w
        _native.check(lib.tgmx_mixer_prologue(a['ex'].data_ptr(), a['seed_t'].data_ptr(), a['nbr_t'].data_ptr(), S, K, D, tw.weight.data_ptr(),
                                              tw.bias.data_ptr(), T, x0.data_ptr(), ldx0, stream), 'tgmx_mixer_prologue')  # fmt: skip
        rows = lambda buf, ld, n=R: buf[: n * ld].view(n, ld)
        pl, ol = self.projection_layer, self.output_layer
        sgemm_ep(rows(x0, ldx0)[:, : D + T], pl.weight.detach(), rows(z, ldz)[:, :D], pl.bias.detach())
        for m in self.mlp_mixers:
            token_block(m, z, ldz, S, z1, y, ldz)
            cf = m.channel_feedforward.ffn
            Hc = cf[0].out_features
            sgemm_ep(rows(y, ldz)[:, :D], cf[0].weight.detach(), rows(h, ldh)[:, :Hc], cf[0].bias.detach(), act=2)
            sgemm_ep(rows(h, ldh)[:, :Hc], cf[3].weight.detach(), rows(z, ldz)[:, :D], cf[3].bias.detach(), res=rows(z1, ldz)[:, :D])
        s = a['seeds']
        _native.check(
            lib.tgmx_mixer_tail(z.data_ptr(), ldz, S, K, D, a['nids'].data_ptr(), a['node_x'].data_ptr(), a['node_x'].shape[0], self.node_dim,
                                a['tg_nbr'].data_ptr(), a['tg_lo'].data_ptr(), a['tg_cnt'].data_ptr(), s[0].data_ptr(), s[0].numel(),
                                s[1].data_ptr(), s[1].numel(), s[2].data_ptr(), cat.data_ptr(), ldcat, stream),
            'tgmx_mixer_tail',
        )  # fmt: skip
        sgemm_ep(rows(cat, ldcat, S)[:, : D + self.node_dim], ol.weight.detach(), out, ol.bias.detach())
        return out

    def _weights(self) -> tuple:
        """(argument block with the weights filled in, the tensors it points at), cached against the parameters' versions."""

        def build(f32) -> '_native.GraphMixerFwd':
            blk = _native.GraphMixerFwd()
            tw = self.time_encoder.w
            blk.tw, blk.tb = f32(tw.weight.reshape(-1)), f32(tw.bias)
            blk.proj_w, blk.proj_b = f32(self.projection_layer.weight), f32(self.projection_layer.bias)
            blk.out_w, blk.out_b = f32(self.output_layer.weight), f32(self.output_layer.bias)
            blk.num_layers, blk.eps = self.num_layers, fill_mixer_layers(blk, self.mlp_mixers, f32, 'GraphMixerEncoder')
            blk.K, blk.D, blk.T, blk.E, blk.F = self.num_tokens, self.edge_dim, self.time_dim, self.embed_dim, self.node_dim
            return blk

        return cached_block(self, build)

    def _forward_native(self, a: dict) -> Tensor:
        blk, _ = self._weights()
        S = a['S']
        dev = a['ex'].device
        out = torch.empty((S, self.embed_dim), dtype=torch.float32, device=dev)
        if S == 0:
            return out
        d = self._dims(S)
        x0, z, z1, y, h, cat = self._scratch(S, dev)
        blk.nbr_edge_x, blk.seed_t, blk.nbr_t, blk.nbr_nids = a['ex'].data_ptr(), a['seed_t'].data_ptr(), a['nbr_t'].data_ptr(), a['nids'].data_ptr()
        for g, t in enumerate(a['seeds']):
            blk.seeds[g], blk.n_seeds[g] = t.data_ptr(), t.numel()
        blk.tg_nbr, blk.tg_lo, blk.tg_cnt = a['tg_nbr'].data_ptr(), a['tg_lo'].data_ptr(), a['tg_cnt'].data_ptr()
        blk.node_x, blk.num_nodes, blk.S = a['node_x'].data_ptr(), a['node_x'].shape[0], S
        blk.x0, blk.z, blk.z1, blk.y, blk.h, blk.cat = x0.data_ptr(), z.data_ptr(), z1.data_ptr(), y.data_ptr(), h.data_ptr(), cat.data_ptr()
        blk.ldx0, blk.ldz, blk.ldh, blk.ldcat = d['ldx0'], d['ldz'], d['ldh'], d['ldcat']
        blk.out = out.data_ptr()
        check_supported(_native.load().tgmx_graphmixer_forward(ctypes.byref(blk), _native.stream_ptr()), 'tgmx_graphmixer_forward')
        return out
