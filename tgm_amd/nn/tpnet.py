"""``RandomProjectionModule`` and ``TPNet`` (tgm/nn/encoder/tpnet.py; https://arxiv.org/abs/2410.04013) -- same constructor arguments,
defaults, errors and ``state_dict`` layout (``beginning_time``, ``now_time``, ``random_projections.{0..L}``, ``mlp.{0,2}.*``;
``time_encoder.w.*``, ``random_projections.*``, ``projection_layer.{0,2}.*``, ``mlp_mixers.{i}.*``): a checkpoint of the reference's
example loads with ``strict=True``, and back.

``RandomProjectionModule`` keeps the temporal walk matrices A^(0)(t) .. A^(L)(t) as L + 1 tables [num_nodes, dim] of random projections.

* ``update(src, dst, time)`` is ONE native call (``tgmx_tpnet_update``) and deterministic: the batch's messages are staged from the
  tables as they were before the batch (level i reads the decayed ``P[i-1]`` before this batch adds to it, as the reference's descending
  loop does), then every table element is rescaled and receives its row's messages in batch order (all sources, then all destinations)
  by exactly one thread.  No float atomics: two runs from the same state give the same bits.  The decay is applied eagerly, so the
  tables always hold the materialised values.  Edges with an endpoint outside ``[0, num_nodes)`` contribute nothing.
* ``forward(src, dst)`` is one kernel (``tgmx_tpnet_pair_features``: gather, Gram matrix, clamp and ``log(x + 1)``) plus the small MLP
  on the exact-fp32 MFMA GEMM.  ``[P, 2 L + 2, dim]`` is never stored.  A negative id indexes from the end, as torch indexing does in
  the reference: ``PADDED_NODE_ID`` (-1) is the LAST table row.

``TPNet.forward(node_x, edge_index, edge_time, neighbours, neighbours_time, neighbours_edge_feat) -> (z_src, z_dst)``: rows ``[:B]`` of
the three neighbour tensors belong to ``edge_index[0]``, rows ``[B:2B]`` to ``edge_index[1]``.  Every neighbour slot becomes a token
``[node_x[nbr] | cos(w log(dt + 1) + b) | edge features | pair(nbr, src) | pair(nbr, dst)]`` -> Linear, ReLU, Linear -> MLPMixer layers
-> mean over the slots.  Two quirks of the reference are part of the contract:

* its ``embeddings.masked_fill(...)`` after the projection discards the result, so pad tokens are NOT zeroed there (their node and time
  columns are zero, their edge features are whatever the sampler wrote, and they go through the projection's biases like any token);
* pad slots carry the pair features of node ``num_nodes - 1`` (id -1 indexes the last table row).

``encode_pairs(node_x, src, dst, edge_time, nbr_nids, nbr_edge_time, nbr_edge_x, src_rows, dst_rows)`` is the same computation reading
hop 0 of the sampler's batch in place: ``src_rows`` / ``dst_rows`` [B] index its rows (what ``batch.seed_node_nbr_mask[...]`` holds), for
one negative per positive as for one-vs-many, so the example's ``repeat_interleave`` / ``repeat`` / ``cat`` copies of ``nbr_edge_x`` & co.
are never made.  ``forward`` is ``encode_pairs`` with identity rows; the results are identical bit for bit.

Inference (no gradient needed, no active dropout) is ONE native call, ``tgmx_tpnet_forward``.  Training (gradients enabled and a parameter
that wants one) is native too: the saving forward ``tgmx_tpnet_forward_train`` (the bits of the inference call when dropout is off) and
ONE backward call, ``tgmx_tpnet_backward``, behind a ``torch.autograd.Function`` (``_tpnet_train.py``; ``TGMX_TPNET_BWD=torch`` keeps the
composed path).  Outside that envelope -- autocast, ``node_x`` or the edge features asking for a gradient, train-mode dropout with no
parameter to train -- the same arithmetic is composed from torch ops on the device under autograd, with the same parameters.  A
shape outside the native envelope (more than 4 tables, i.e. ``num_layer > 3``; more than 8 mixer layers; a token block that does not fit
LDS; a time encoder that is not ``Time2Vec``) also takes the composed path on the device.  CPU tensors raise ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes
import math
import warnings
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .. import _native
from ..constants import PADDED_NODE_ID
from . import _ops, _tpnet_train
from ._fwd_plumbing import Unsupported, cached_block, carve_scratch, check_supported, fill_mixer_layers, i32, i64, needs_torch, pair_inputs, up4
from ._paramver import TransientCaches
from .mlp_mixer import MLPMixer, sgemm_ep
from .time_encoding import Time2Vec


class RandomProjectionModule(TransientCaches, nn.Module):
    r"""Temporal walk matrices $A^{(0)}(t), \dots, A^{(k)}(t)$ maintained through random feature propagation, and the pairwise features
    read from them; see the module docstring for what runs natively.

    Args (the reference's): num_nodes, num_layer (max hop), time_decay_weight (lambda), beginning_time, use_matrix (dim = num_nodes,
    P[0] the identity), scale_random_projection (clamp + log), enforce_dim, num_edges and dim_factor
    (dim = min(int(log(2 num_edges)) dim_factor, num_nodes)), concat_src_dst (the (2L+2)^2 Gram of the stacked rows, or the (L+1)^2 cross
    products), device.
    """

    def __init__(self, num_nodes: int, num_layer: int, time_decay_weight: float, beginning_time: float, use_matrix: bool = True,
                 scale_random_projection: bool = True, enforce_dim: int | None = None, num_edges: int | None = None,
                 dim_factor: int | None = None, concat_src_dst: bool = True, device: str = 'cpu') -> None:  # fmt: skip
        super().__init__()
        if not use_matrix:
            if enforce_dim is not None:
                self.dim = enforce_dim
            elif num_edges is not None and dim_factor is not None:
                self.dim = min(int(math.log(num_edges * 2)) * dim_factor, num_nodes)
            else:
                raise ValueError('When `use_matrix` is False, either providing enforce_dim or both num_edges and dim_factor')
        else:
            self.dim = num_nodes
        self.num_nodes = num_nodes
        self.num_layer = num_layer
        self.time_decay_weight = time_decay_weight
        self.use_matrix = use_matrix
        self.device = device
        self.scale = scale_random_projection
        self.concat_src_dst = concat_src_dst

        self.beginning_time = nn.Parameter(torch.tensor(beginning_time), requires_grad=False)
        self.now_time = nn.Parameter(torch.tensor(beginning_time), requires_grad=False)
        self.random_projections = nn.ParameterList()
        for i in range(self.num_layer + 1):
            if i > 0:
                t = torch.zeros_like(self.random_projections[i - 1])
            elif use_matrix:
                t = torch.eye(self.dim)
            else:
                t = torch.normal(0, 1 / math.sqrt(self.dim), (num_nodes, self.dim))
            self.random_projections.append(nn.Parameter(t, requires_grad=False))
        self.out_dim = (2 * self.num_layer + 2) ** 2 if concat_src_dst else (self.num_layer + 1) ** 2
        self.mlp = nn.Sequential(nn.Linear(self.out_dim, self.out_dim * 4), nn.ReLU(), nn.Linear(self.out_dim * 4, self.out_dim))

    # -- native plumbing -----------------------------------------------------------------------------------------------------------------
    def _tables(self) -> '_native.TPNetTables':
        tb = _native.TPNetTables()
        if self.num_layer + 1 > _native.TPNET_MAX_LEVELS:
            raise NotImplementedError(f'tgm_amd RandomProjectionModule: at most {_native.TPNET_MAX_LEVELS - 1} layers on the native path')
        shape = tuple(self.random_projections[0].shape)
        for i, p in enumerate(self.random_projections):
            _native.require_device(p, f'random_projections[{i}]')
            if p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape) != shape or p.dim() != 2:
                raise ValueError(f'random_projections[{i}] must be a contiguous float32 [{shape[0]}, {shape[1]}] tensor, got {p.dtype} {list(p.shape)}')
            tb.P[i] = p.data_ptr()
        tb.levels, tb.num_nodes, tb.dim = self.num_layer + 1, shape[0], shape[1]
        return tb

    def _mlp_needs_grad(self) -> bool:
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.mlp.parameters())

    def _pair_features(self, a: Tensor, a_rows: Optional[Tensor], a_num_rows: int, k: int, b0: Tensor, b1: Optional[Tensor], bmod: int, n: int,
                       out: Tensor, ldo: int) -> None:  # fmt: skip
        tb = self._tables()
        check_supported(
            _native.load().tgmx_tpnet_pair_features(ctypes.byref(tb), a.data_ptr(), _native.ptr(a_rows), a_num_rows, k, b0.data_ptr(), _native.ptr(b1),
                                                    bmod, n, int(self.concat_src_dst), int(self.scale), out.data_ptr(), ldo, _native.stream_ptr()),
            'tgmx_tpnet_pair_features',
        )  # fmt: skip

    def random_feature(self, src: Tensor, dst: Tensor) -> Tensor:
        """[P, out_dim]: the pair features before the MLP (the native kernel alone)."""
        _native.require_device(src, 'src')
        _native.require_device(dst, 'dst')
        a, b = i32(src.reshape(-1)), i32(dst.reshape(-1))
        if a.numel() != b.numel():
            raise ValueError('src and dst must have one entry per pair')
        n, ld = a.numel(), up4(self.out_dim)
        feat = torch.empty((n, ld), dtype=torch.float32, device=a.device)
        if n:
            self._pair_features(a, None, n, 1, b, None, n, n, feat, ld)
        return feat[:, : self.out_dim]

    # -- the reference's interface ---------------------------------------------------------------------------------------------------------
    def forward(self, src: Tensor, dst: Tensor) -> Tensor:
        """Pairwise features of (src[p], dst[p]) -> [P, out_dim]."""
        _native.require_device(src, 'src')
        _native.require_device(dst, 'dst')
        if self._mlp_needs_grad() or self.num_layer + 1 > _native.TPNET_PAIR_MAX_LEVELS:
            return self._torch_forward(src, dst)
        feat = self.random_feature(src, dst)
        n, od = feat.shape[0], self.out_dim
        out = torch.empty((n, od), dtype=torch.float32, device=feat.device)
        if n:
            h = torch.empty((n, 4 * od), dtype=torch.float32, device=feat.device)
            sgemm_ep(feat, _ops._f32c(self.mlp[0].weight.detach(), 'mlp.0.weight'), h, _ops._f32c(self.mlp[0].bias.detach(), 'mlp.0.bias'), act=1)
            sgemm_ep(h, _ops._f32c(self.mlp[2].weight.detach(), 'mlp.2.weight'), out, _ops._f32c(self.mlp[2].bias.detach(), 'mlp.2.bias'))
        return out

    def _torch_forward(self, src: Tensor, dst: Tensor) -> Tensor:
        """The same from torch ops (autograd-capable for the MLP; not native)."""
        s, d = self.get_random_projections(src.long()), self.get_random_projections(dst.long())
        if self.concat_src_dst:
            rp = torch.cat([s, d], dim=1)
            f = torch.matmul(rp, rp.transpose(1, 2)).reshape(src.shape[0], -1)
        else:
            f = torch.matmul(s, d.transpose(1, 2)).reshape(src.shape[0], -1)
        if self.scale:
            f = torch.log(f.masked_fill(f < 0, 0.0) + 1.0)
        return self.mlp(f)

    def update(self, src: Tensor, dst: Tensor, time: Tensor) -> None:
        """Update the temporal walk matrices after observing a batch of interactions (one native call, deterministic)."""
        for name, t in (('src', src), ('dst', dst), ('time', time), ('now_time', self.now_time)):
            _native.require_device(t, name)
        tb = self._tables()
        s, d, t = i32(src.reshape(-1)), i32(dst.reshape(-1)), i64(time.reshape(-1))
        n = s.numel()
        if d.numel() != n or t.numel() != n:
            raise ValueError('src, dst and time must have one entry per edge')
        if n == 0:
            return
        dev = s.device
        st = self.__dict__
        head = st.get('_tgmx_head')
        if head is None or head.numel() != tb.num_nodes or head.device != dev:
            head = st['_tgmx_head'] = torch.full((tb.num_nodes,), _native.TPNET_HEAD_EMPTY, dtype=torch.int32, device=dev)
        need = max(1, self.num_layer * 2 * n * tb.dim)
        msg = st.get('_tgmx_msg')
        if msg is None or msg.numel() < need or msg.device != dev:
            msg = st['_tgmx_msg'] = torch.empty(need, dtype=torch.float32, device=dev)
        now = self.now_time.data
        if now.dtype == torch.int64 and now.is_contiguous():
            now_in, now_out, is_f64 = now, now, 0
        else:  # a float beginning_time: the first update turns now_time into the int64 time of the batch, as the reference's does
            now_in, now_out, is_f64 = now.reshape(-1)[:1].to(torch.float64), torch.empty((), dtype=torch.int64, device=dev), 1
        rc = (
            _native.load().tgmx_tpnet_update(ctypes.byref(tb), s.data_ptr(), d.data_ptr(), t.data_ptr(), n, float(self.time_decay_weight), now_in.data_ptr(),
                                             is_f64, now_out.data_ptr(), msg.data_ptr(), head.data_ptr(), _native.stream_ptr())
        )  # fmt: skip
        if rc != 0:
            st.pop('_tgmx_head', None)  # a call that stopped between its two launches leaves marks behind: start from a clean array next time
        _native.check(rc, 'tgmx_tpnet_update')
        if now_out is not now:
            self.now_time.data = now_out

    def get_random_projections(self, node_ids: Tensor) -> Tensor:
        """[len(node_ids), L + 1, dim]: the random projections of the given nodes."""
        return torch.stack([self.random_projections[i][node_ids] for i in range(self.num_layer + 1)], dim=1)

    def reset_random_projections(self, reset_zero: bool = True) -> None:
        for i in range(1, self.num_layer + 1):
            nn.init.zeros_(self.random_projections[i])
        self.now_time.data = self.beginning_time.data.clone()
        if not self.use_matrix and reset_zero:
            nn.init.normal_(self.random_projections[0], mean=0, std=1 / math.sqrt(self.dim))

    def backup_random_projections(self) -> Tuple[Tensor, List]:
        return self.now_time.clone(), [self.random_projections[i].clone() for i in range(1, self.num_layer + 1)]

    def reload_random_projections(self, random_projections: Tuple) -> None:
        if len(random_projections) != 2:
            raise ValueError('Expected a tuple of (now_time, random_projections)')
        now_time, random_projections = random_projections
        if not torch.is_tensor(now_time):
            raise ValueError(f'now time must be a torch.Tensor, got: {type(now_time)}')
        if len(random_projections) != self.num_layer:
            raise ValueError(f'len(random_projections) ({len(random_projections)}) != self.num_layer ({self.num_layer})')
        self.now_time.data = now_time.clone()
        for i in range(1, self.num_layer + 1):
            if not torch.is_tensor(random_projections[i - 1]):
                raise ValueError(f'random_projections[{i - 1}] must be a torch.Tensor, got: {type(random_projections[i - 1])}')
            self.random_projections[i].data = random_projections[i - 1].clone()


class TPNet(TransientCaches, nn.Module):
    r"""TPNet (https://arxiv.org/abs/2410.04013); see the module docstring for the interface, the two reference quirks that are part of the
    contract (pad tokens are not zeroed after the projection; pad slots carry the pair features of node ``num_nodes - 1``) and for what
    runs natively."""

    def __init__(self, node_feat_dim: int, edge_x_dim: int, time_feat_dim: int, output_dim: int, num_neighbors: int, num_layers: int = 2,
                 dropout: float = 0.1, random_projections: RandomProjectionModule | None = None, device: str = 'cpu',
                 time_encoder: Callable[..., nn.Module] = Time2Vec) -> None:  # fmt: skip
        super().__init__()
        self.device = device
        self.node_feat_dim, self.edge_x_dim, self.time_feat_dim, self.output_dim = node_feat_dim, edge_x_dim, time_feat_dim, output_dim
        self.num_layers, self.dropout = num_layers, dropout
        self.time_encoder = time_encoder(time_feat_dim).to(device)
        self.random_projections = random_projections
        self.num_neighbors = num_neighbors
        self.random_feature_dim = 0 if random_projections is None else random_projections.out_dim * 2
        self.projection_layer = nn.Sequential(
            nn.Linear(node_feat_dim + edge_x_dim + time_feat_dim + self.random_feature_dim, output_dim * 2), nn.ReLU(), nn.Linear(output_dim * 2, output_dim)
        ).to(device)
        self.mlp_mixers = nn.ModuleList([
            MLPMixer(num_tokens=num_neighbors, num_channels=output_dim, token_dim_expansion_factor=0.5, channel_dim_expansion_factor=4.0, dropout=dropout).to(device)
            for _ in range(num_layers)
        ])  # fmt: skip

    # -- inputs ------------------------------------------------------------------------------------------------------------------------
    def _check_slots(self, k: int) -> None:
        if k != self.num_neighbors:
            raise ValueError(f'TPNet(num_neighbors={self.num_neighbors}) got {k} neighbour slots per row')

    def _inputs(self, *tensors) -> dict:
        """(node_x, src, dst, edge_time, nids, nbr_t, nbr_x, src_rows, dst_rows), checked and converted."""
        a = pair_inputs(*tensors, self.node_feat_dim, self.edge_x_dim, self._check_slots, 'B')
        src_rows, dst_rows = a.pop('src_rows'), a.pop('dst_rows')
        return dict(a, rows=None if src_rows is None else torch.cat([src_rows, dst_rows]), B=a['src'].numel(), k=a['nids'].shape[1])

    def forward(self, node_x: Tensor, edge_index: Tensor, edge_time: Tensor, neighbours: Tensor, neighbours_time: Tensor,
                neighbours_edge_feat: Tensor) -> Tuple[Tensor, Tensor]:  # fmt: skip
        return self._run(self._inputs(node_x, edge_index[0], edge_index[1], edge_time, neighbours, neighbours_time, neighbours_edge_feat, None, None))

    def encode_pairs(self, node_x: Tensor, src: Tensor, dst: Tensor, edge_time: Tensor, nbr_nids: Tensor, nbr_edge_time: Tensor, nbr_edge_x: Tensor,
                     src_rows: Tensor, dst_rows: Tensor) -> Tuple[Tensor, Tensor]:  # fmt: skip
        """``forward`` on ``nbr_*[cat(src_rows, dst_rows)]`` without making those copies (same results, bit for bit)."""
        return self._run(self._inputs(node_x, src, dst, edge_time, nbr_nids, nbr_edge_time, nbr_edge_x, src_rows, dst_rows))

    def _native_ok(self) -> bool:
        rp = self.random_projections
        return (hasattr(self.time_encoder, 'w') and self.num_layers <= _native.MIXER_MAX_LAYERS
                and (rp is None or rp.num_layer + 1 <= _native.TPNET_PAIR_MAX_LEVELS))  # fmt: skip

    def _run(self, a: dict) -> Tuple[Tensor, Tensor]:
        if needs_torch(self, self.dropout, a['node_x'], a['nbr_x']):
            if _tpnet_train.in_envelope(self, a):
                try:
                    return _tpnet_train.apply(self, a)
                except Unsupported:  # the token block does not fit the training kernels: compose
                    pass
            return self._torch_forward(a)
        if not self._native_ok():
            self._warn_composed('its shape is outside the native envelope (num_layer <= 3, at most 8 mixer layers, Time2Vec)')
            return self._torch_forward(a)
        for m in self.mlp_mixers:
            m._check_native()
        B = a['B']
        out = torch.empty((2 * B, self.output_dim), dtype=torch.float32, device=a['node_x'].device)
        if B:
            try:
                self._forward_native(a, out)
            except Unsupported as e:  # the token block does not fit LDS: compose
                self._warn_composed(str(e))
                return self._torch_forward(a)
        return out[:B], out[B:]

    def _warn_composed(self, why: str) -> None:
        if not self.__dict__.get('_tgmx_warned'):
            self.__dict__['_tgmx_warned'] = True
            warnings.warn(f'tgm_amd TPNet: inference runs as torch ops on the device, not natively: {why}', RuntimeWarning, stacklevel=3)

    # -- training / outside the native envelope: torch ops under autograd (not native) ---------------------------------------------------
    def _torch_forward(self, a: dict) -> Tuple[Tensor, Tensor]:
        B, k = a['B'], a['k']
        dev = a['node_x'].device
        rows = torch.arange(2 * B, device=dev) if a['rows'] is None else a['rows'].long()
        nids = a['nids'][rows].long()  # [2B, k]: sources, then destinations
        pad = (nids == PADDED_NODE_ID).unsqueeze(-1)
        node = a['node_x'][nids].masked_fill(pad, 0.0)
        t2 = torch.cat([a['t'], a['t']])
        lg = torch.log((t2[:, None] - a['nbr_t'][rows]) + 1)  # float32 log of the int64 gap + 1, as the reference takes it
        tw = getattr(self.time_encoder, 'w', None)
        time = torch.cos(F.linear(lg.unsqueeze(-1).float(), tw.weight, tw.bias)) if tw is not None else self.time_encoder(lg)
        feats = [node, time.masked_fill(pad, 0.0), a['nbr_x'][rows]]
        rp = self.random_projections
        if rp is not None:
            flat = nids.reshape(-1)
            src2, dst2 = a['src'].long().repeat(2).repeat_interleave(k), a['dst'].long().repeat(2).repeat_interleave(k)
            feats += [rp._torch_forward(flat, src2).reshape(2 * B, k, -1), rp._torch_forward(flat, dst2).reshape(2 * B, k, -1)]
        z = self.projection_layer(torch.cat(feats, dim=2))  # (the reference's masked_fill here discards its result: pads stay as projected)
        for m in self.mlp_mixers:
            z = m._torch_forward(z)
        z = z.mean(dim=1)
        return z[:B], z[B:]

    # -- inference ------------------------------------------------------------------------------------------------------------------------
    def _dims(self) -> dict:
        od = 0 if self.random_projections is None else self.random_projections.out_dim
        E = self.output_dim
        Hc = max(m.channel_feedforward.ffn[0].out_features for m in self.mlp_mixers) if self.num_layers else 4
        return dict(od=od, ldf=up4(max(od, 1)), ldfh=up4(max(4 * od, 1)), ldx0=up4(self.node_feat_dim + self.time_feat_dim + self.edge_x_dim + 2 * od),
                    ldhp=up4(2 * E), ldz=up4(E), ldh=up4(Hc))  # fmt: skip

    def _scratch(self, B: int, k: int, device) -> List[Tensor]:
        """feat, feat_h, pf, x0, hp, z, z1, y, h: views into one buffer kept between batches."""
        d = self._dims()
        R = 2 * B * k
        R2 = 2 * R if d['od'] else 0
        return carve_scratch(self, [R2 * d['ldf'], R2 * d['ldfh'], R2 * d['ldf'], R * d['ldx0'], R * d['ldhp']] + [R * d['ldz']] * 3 + [R * d['ldh']], device)

    def _weights(self) -> tuple:
        """(argument block with the weights filled in, the tensors it points at), cached against the parameters' versions."""

        def build(f32) -> '_native.TPNetFwd':
            blk = _native.TPNetFwd()
            tw, pl, rp = self.time_encoder.w, self.projection_layer, self.random_projections
            blk.tw, blk.tb = f32(tw.weight.reshape(-1)), f32(tw.bias)
            blk.proj_w0, blk.proj_b0, blk.proj_w2, blk.proj_b2 = f32(pl[0].weight), f32(pl[0].bias), f32(pl[2].weight), f32(pl[2].bias)
            if rp is not None:
                blk.rp_w1, blk.rp_b1, blk.rp_w2, blk.rp_b2 = f32(rp.mlp[0].weight), f32(rp.mlp[0].bias), f32(rp.mlp[2].weight), f32(rp.mlp[2].bias)
                blk.rp_concat, blk.rp_scale, blk.rp_out_dim = int(rp.concat_src_dst), int(rp.scale), rp.out_dim
            blk.num_layers, blk.eps = self.num_layers, fill_mixer_layers(blk, self.mlp_mixers, f32, 'TPNet')
            blk.k, blk.dN, blk.dE, blk.dT, blk.E = self.num_neighbors, self.node_feat_dim, self.edge_x_dim, self.time_feat_dim, self.output_dim
            return blk

        return cached_block(self, build)

    def _bind_inputs(self, blk: '_native.TPNetFwd', a: dict) -> None:
        """The caller's tensors and the tables of this call."""
        blk.node_x, blk.num_nodes = a['node_x'].data_ptr(), a['node_x'].shape[0]
        blk.src, blk.dst, blk.edge_time, blk.B = a['src'].data_ptr(), a['dst'].data_ptr(), a['t'].data_ptr(), a['B']
        blk.nbr_nids, blk.nbr_t, blk.nbr_x, blk.S = a['nids'].data_ptr(), a['nbr_t'].data_ptr(), a['nbr_x'].data_ptr(), a['nids'].shape[0]
        blk.rows = _native.ptr(a['rows'])
        if self.random_projections is not None:
            blk.tables = self.random_projections._tables()  # read every call: update / reload may have replaced the tensors
        else:
            blk.tables.levels = 0

    def _forward_native(self, a: dict, out: Tensor) -> None:
        blk, _ = self._weights()
        B, k = a['B'], a['k']
        d = self._dims()
        bufs = self._scratch(B, k, out.device)
        self._bind_inputs(blk, a)
        blk.feat, blk.feat_h, blk.pf, blk.x0, blk.hp, blk.z, blk.z1, blk.y, blk.h = (b.data_ptr() for b in bufs)
        blk.ldf, blk.ldfh, blk.ldx0, blk.ldhp, blk.ldz, blk.ldh = d['ldf'], d['ldfh'], d['ldx0'], d['ldhp'], d['ldz'], d['ldh']
        blk.out = out.data_ptr()
        check_supported(_native.load().tgmx_tpnet_forward(ctypes.byref(blk), _native.stream_ptr()), 'tgmx_tpnet_forward')
