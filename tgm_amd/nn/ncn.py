"""``NCNPredictor`` (tgm/nn/decoder/ncnpred.py; TNCN, https://arxiv.org/abs/2406.07926) -- same constructor arguments, errors, parameter
names, shapes and initialisation order (``xslin.*``, ``xsmlp.{0,2}.*``): a checkpoint of the reference's example loads with
``strict=True``, and back.

``forward(x, edge_index, tar_ei, last_update=None, edge_time=None) -> [B * out_channels]``.  With A the symmetric adjacency of the batch's
sampled subgraph (``A[a, b]`` = how often ``(a, b)`` or ``(b, a)`` occurs in ``edge_index``; a self-loop counts twice), ``R_i[r] = A[tar_i[r]]``,
``I_i[r]`` the ``tar_i[r]``-th unit row, and ``W[r, n] = exp(-(float32(edge_time[r] - last_update[n]) / 10000))`` (1 without
``cn_time_decay``):

    k = 2:  xs = [x[tar_i] * x[tar_j] | ((R_i o R_j) o W) x]
    k = 4:  xs = [x[tar_i] * x[tar_j] | ((I_i o R_j) o W) x | ((R_i o I_j) o W) x | ((R_i o R_j) o W) x]
    out = xsmlp(xs).view(-1)

Three quirks of the reference are part of the contract:

* ``duplicate_targets='last'`` (the default) is what the reference computes on the CPU: its row slicing maps ids to positions with
  ``mapping[rows] = arange(len(rows))``, so of several positions holding one id only the LAST keeps its adjacency (and identity) row,
  on each side.  A source that occurs twice in a training batch, and all but the last candidate of a one-vs-many call, get zero
  common-neighbour blocks.  ``duplicate_targets='all'`` gives every position its row (what the paper describes, and what ``'last'``
  gives for B = 1).  The argument is not part of the ``state_dict``.
* ``xs.relu()`` in the reference discards its result: negative entries of ``xs`` reach the MLP.
* ``xslin`` is in the ``state_dict`` and unused.

``edge_index`` may be int32 or int64, and may be the strided ``ei[:, :E]`` view ``sampled_edge_list`` returns (it is not copied).
``adjacency(num_nodes, edge_index)`` prepares the adjacency once; ``forward`` / ``get_cn_emb`` take the prepared object wherever they take
``edge_index``, so the evaluation loop's one call per positive edge shares one build.  The results are the same bit for bit.

Inference (no gradient needed) is ONE native call, ``tgmx_ncn_forward``: a radix sort of the 2 E half-edges is the adjacency, one wave
per pair intersects two sorted rows and gather-sums ``x`` over the matches in ascending id (deterministic, no float atomics), then the two
Linear layers on the exact-fp32 GEMM.

Training (autograd has something to track) is native too: ``forward`` is the same ``tgmx_ncn_forward`` call, writing what the backward
reads into buffers of the call (so the result is the no-grad call's bit for bit, and the positives' and negatives' calls of one step do
not share them), and the backward is ONE native call, ``tgmx_ncn_backward`` (``_ncn_train.py``, ``csrc/ncn_bwd.hip``): the two Linear layers
from the shared blocks, then ``dx`` node by node through two inverted indexes of the pairs and the forward's adjacency -- fixed summation
order, no float atomics, no ``[B, N]`` intermediates.  ``last_update`` / ``edge_time`` get no gradient (the decay weight depends on integers
only) and ``xslin`` gets ``None``.  Outside that path -- autocast, parameters of another dtype, ``get_cn_emb`` under gradients,
``TGMX_NCN_BWD=torch`` -- the same arithmetic is composed from torch ops on the device under autograd, through dense ``[B, N]`` rows (never
``[N, N]``).  ``TGMX_NCN_BWD=py`` issues the native backward's launches one ctypes call each (the same bits).

``k = 8`` is accepted by the constructor and not implemented: ``forward`` raises ``NotImplementedError``.  CPU tensors raise
``NativeLibraryError``.  A pair with a target id outside ``[0, N)`` gives a zero row, and no gradient, on every path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from . import _ncn_train, _ops
from ._fwd_plumbing import cached_block, carve_scratch, i64, needs_torch, up4
from ._paramver import TransientCaches


class PreparedAdjacency:
    """The sorted-row adjacency of one ``edge_index`` on the device (``adjacency()``): opaque to callers."""

    __slots__ = ('indptr', 'cols', 'num_nodes', 'num_edges')

    def __init__(self, indptr: Tensor, cols: Tensor, num_nodes: int, num_edges: int) -> None:
        self.indptr, self.cols, self.num_nodes, self.num_edges = indptr, cols, num_nodes, num_edges


def _edge_view(edge_index: Tensor) -> Tuple[Tensor, int, int]:
    """(tensor whose rows the kernels can walk, is64, row stride): int32 / int64 [2, E] with unit inner stride is taken as it is."""
    _native.require_device(edge_index, 'edge_index')
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f'expected edge_index [2, E], got {list(edge_index.shape)}')
    if edge_index.dtype not in (torch.int32, torch.int64):
        edge_index = edge_index.long()
    E = edge_index.shape[1]
    if E > 0 and (edge_index.stride(1) != 1 or edge_index.stride(0) < E):  # (also an expanded or overlapping view: rows closer than E)
        edge_index = edge_index.contiguous()
    return edge_index, int(edge_index.dtype == torch.int64), max(edge_index.stride(0), E, 1)


def _adj_ws_bytes(E: int) -> int:
    need = int(_native.load().tgmx_ncn_adj_workspace_bytes(E))  # host arithmetic only: no launch
    if need == 0:
        raise ValueError(f'NCNPredictor: {E} edges are more than the adjacency build indexes (2 E < 2^31)')
    return need


def adjacency(num_nodes: int, edge_index: Tensor) -> PreparedAdjacency:
    """Prepare the adjacency of ``edge_index`` over ``num_nodes`` local ids once (``tgmx_ncn_adj_build``), for any number of decoder calls."""
    ei, is64, stride = _edge_view(edge_index)
    E, dev = ei.shape[1], ei.device
    if num_nodes < 1:
        raise ValueError('adjacency: num_nodes must be positive')
    indptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    cols = torch.empty(max(2 * E, 1), dtype=torch.int32, device=dev)
    need = _adj_ws_bytes(E)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _native.check(_native.load().tgmx_ncn_adj_build(ei.data_ptr(), is64, stride, E, num_nodes, indptr.data_ptr(), cols.data_ptr(), ws.data_ptr(),
                                                    need, _native.stream_ptr()), 'tgmx_ncn_adj_build')  # fmt: skip
    return PreparedAdjacency(indptr, cols, num_nodes, E)


class NCNPredictor(TransientCaches, nn.Module):
    r"""Temporal Neural Common Neighbor decoder; see the module docstring for the arithmetic, the reference's quirks that are part of the
    contract and for what runs natively.

    Args (the reference's): in_channels, hidden_dim, out_channels, k (2 / 4 / 8: the hops of common-neighbour extraction; 8 is not
    implemented), cn_time_decay.  ``duplicate_targets``: ``'last'`` (the reference's CPU behaviour) or ``'all'``.
    """

    def __init__(self, in_channels: int, hidden_dim: int, out_channels: int, k: int = 2, cn_time_decay: bool = False, *,
                 duplicate_targets: str = 'last') -> None:  # fmt: skip
        super().__init__()
        if k not in [2, 4, 8]:
            raise ValueError('Please choose k from [2,4,8]')
        if duplicate_targets not in ('last', 'all'):
            raise ValueError(f"duplicate_targets must be 'last' or 'all', got {duplicate_targets!r}")
        self.k = k
        self.xslin = nn.Linear(k * in_channels, out_channels)
        self.xsmlp = nn.Sequential(nn.Linear(k * in_channels, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, out_channels))
        self.cn_time_decay = cn_time_decay
        self.duplicate_targets = duplicate_targets
        self.in_channels, self.hidden_dim, self.out_channels = in_channels, hidden_dim, out_channels

    adjacency = staticmethod(adjacency)

    # -- inputs ------------------------------------------------------------------------------------------------------------------------
    def _inputs(self, x: Tensor, edge_index: Union[Tensor, PreparedAdjacency], tar_ei: Tensor, last_update: Optional[Tensor],
                edge_time: Optional[Tensor]) -> dict:  # fmt: skip
        if self.cn_time_decay and (last_update is None or edge_time is None):
            raise RuntimeError('Please provide time_information to perform time decay')
        if self.k == 8:
            raise NotImplementedError('tgm_amd NCNPredictor: k = 8 is not implemented (k = 2 and k = 4 are)')
        _native.require_device(x, 'x')
        _native.require_device(tar_ei, 'tar_ei')
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f'expected x [N, {self.in_channels}], got {list(x.shape)}')
        if tar_ei.dim() != 2 or tar_ei.shape[0] != 2:
            raise ValueError(f'expected tar_ei [2, B], got {list(tar_ei.shape)}')
        N, B = x.shape[0], tar_ei.shape[1]
        if N < 1:
            raise ValueError('x holds no node')
        if tar_ei.dtype not in (torch.int32, torch.int64):
            tar_ei = tar_ei.long()
        if not tar_ei.is_contiguous():
            tar_ei = tar_ei.contiguous()
        a = dict(x=_ops._f32c(x, 'x'), N=N, B=B, tar=tar_ei, lu=None, et=None)
        if isinstance(edge_index, PreparedAdjacency):
            if edge_index.num_nodes != N or edge_index.indptr.device != x.device:
                raise ValueError(f'the prepared adjacency covers {edge_index.num_nodes} nodes on {edge_index.indptr.device}, x has {N} on {x.device}')
            a.update(adj=edge_index, ei=None)
        else:
            ei, is64, stride = _edge_view(edge_index)
            a.update(adj=None, ei=ei, ei_is64=is64, ei_stride=stride)
        if self.cn_time_decay:
            _native.require_device(last_update, 'last_update')
            _native.require_device(edge_time, 'edge_time')
            if last_update.numel() != N or edge_time.numel() != B:
                raise ValueError(f'expected last_update [{N}] and edge_time [{B}], got {list(last_update.shape)} and {list(edge_time.shape)}')
            a.update(lu=i64(last_update.reshape(-1)), et=i64(edge_time.reshape(-1)))
        return a

    # -- the reference's interface -------------------------------------------------------------------------------------------------------
    def get_cn_emb(self, x: Tensor, edge_index: Union[Tensor, PreparedAdjacency], tar_ei: Tensor,
                   time_info: Tuple[Optional[Tensor], Optional[Tensor]]) -> Tensor:  # fmt: skip
        """The common-neighbour embeddings of every pair: [B, (k - 1) in_channels]."""
        a = self._inputs(x, edge_index, tar_ei, time_info[0], time_info[1])
        if needs_torch(self, 0.0, x):
            return self._torch_xs(a)[:, self.in_channels :]
        xs, _ = self._native_xs(a, mlp=False)
        return xs[:, self.in_channels : self.k * self.in_channels].clone()

    def forward(self, x: Tensor, edge_index: Union[Tensor, PreparedAdjacency], tar_ei: Tensor, last_update: Optional[Tensor] = None,
                edge_time: Optional[Tensor] = None) -> Tensor:  # fmt: skip
        a = self._inputs(x, edge_index, tar_ei, last_update, edge_time)
        if needs_torch(self, 0.0, x):
            if _ncn_train.in_envelope(self, a['x']):
                return _ncn_train.apply(self, a)
            # (the reference's xs.relu() discards its result)
            return self.xsmlp(self._torch_xs(a)).view(-1)
        return self._native_xs(a, mlp=True)[1].view(-1)

    # -- the composed path: torch ops under autograd ---------------------------------------------------------------------------------------
    def _torch_rows(self, a: dict) -> Tuple[Tensor, Tensor]:
        """(half-edge rows, half-edge columns) int64 [2 E]; a half-edge with an endpoint outside [0, N) is left out or gets row N."""
        if a['adj'] is not None:
            # all 2 E slots, with no device -> host read of how many the build kept: a slot behind the last row gets row N, which matches no
            # target, so whatever column it holds (clamped into range) adds zero
            adj = a['adj']
            slots = torch.arange(2 * adj.num_edges, dtype=torch.int32, device=adj.indptr.device)
            rows = torch.searchsorted(adj.indptr[1:], slots, right=True)
            return rows, adj.cols[: slots.numel()].long().clamp(0, a['N'] - 1)
        ei = a['ei'].long()
        ok = ((ei >= 0) & (ei < a['N'])).all(dim=0)
        ei = ei[:, ok]
        return torch.cat([ei[0], ei[1]]), torch.cat([ei[1], ei[0]])

    def _torch_xs(self, a: dict) -> Tensor:
        x, N, B = a['x'], a['N'], a['B']
        dev = x.device
        ti, tj = a['tar'][0].long(), a['tar'][1].long()
        hrow, hcol = self._torch_rows(a)
        ar = torch.arange(B, device=dev)
        # a pair with a target outside [0, N) gets a zero row and marks no last occurrence on either side, as on the native path (no device -> host read)
        inside = lambda t: (t >= 0) & (t < N)
        ok = inside(ti) & inside(tj)
        ti, tj = ti.clamp(0, N - 1), tj.clamp(0, N - 1)

        def rows_of(t: Tensor) -> Tuple[Tensor, Tensor]:
            keep = ok
            if self.duplicate_targets == 'last':
                last = torch.full((N,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, t, torch.where(ok, ar, -1), 'amax')
                keep = ok & (last[t] == ar)
            R = torch.zeros((B, N), dtype=torch.float32, device=dev)
            if hrow.numel():
                R.index_add_(1, hcol, (hrow[None, :] == t[:, None]).float())  # [B, 2 E] -> [B, N]: counts, exact in float32
            I = torch.zeros((B, N), dtype=torch.float32, device=dev)
            I[ar, t] = 1.0
            return R * keep[:, None], I * keep[:, None]

        Ri, Ii = rows_of(ti)
        Rj, Ij = rows_of(tj)
        W = torch.exp(-((a['et'][:, None] - a['lu'][None, :]).to(torch.float32) / 10000)) if self.cn_time_decay else None
        blocks = [(Ri * Rj)] if self.k == 2 else [Ii * Rj, Ri * Ij, Ri * Rj]
        cn = [(b * W if W is not None else b) @ x for b in blocks]
        return torch.cat([x[ti] * x[tj] * ok[:, None]] + cn, dim=-1)

    # -- inference ------------------------------------------------------------------------------------------------------------------------
    def _weights(self) -> tuple:
        def build(f32) -> '_native.NCNFwd':
            blk = _native.NCNFwd()
            m = self.xsmlp
            blk.w1, blk.b1, blk.w2, blk.b2 = f32(m[0].weight), f32(m[0].bias), f32(m[2].weight), f32(m[2].bias)
            blk.C, blk.k, blk.H, blk.out_ch = self.in_channels, self.k, self.hidden_dim, self.out_channels
            return blk

        return cached_block(self, build)

    def _native_xs(self, a: dict, mlp: bool) -> Tuple[Tensor, Optional[Tensor]]:
        """(xs [B, ldxs] scratch view, out [B, out_channels] or None): ``tgmx_ncn_forward``, or its first two stages for ``get_cn_emb``."""
        blk, _ = self._weights()
        lib = _native.load()
        x, N, B, C = a['x'], a['N'], a['B'], self.in_channels
        dev = x.device
        ldxs, ldh = up4(self.k * C), up4(self.hidden_dim)
        adj = a['adj']
        E = adj.num_edges if adj is not None else a['ei'].shape[1]
        need = 0 if adj is not None else _adj_ws_bytes(E)
        own = 0 if adj is not None else (N + 1) + max(2 * E, 1)
        # floats and int32 share the scratch buffer: xs, h, last [2 N], then (without a prepared adjacency) indptr, cols, the sort's workspace
        xs, h, last, ints, ws = carve_scratch(self, [B * ldxs, B * ldh, 2 * N, own, (need + 3) // 4], dev)
        blk.x, blk.N = x.data_ptr(), N
        blk.decay, blk.dup_all = int(self.cn_time_decay), int(self.duplicate_targets == 'all')
        if adj is not None:
            blk.edge_index, blk.E, blk.have_adj = 0, E, 1
            blk.indptr, blk.cols = adj.indptr.data_ptr(), adj.cols.data_ptr()
        else:
            blk.edge_index, blk.ei_stride, blk.E, blk.ei_is64, blk.have_adj = a['ei'].data_ptr(), a['ei_stride'], E, a['ei_is64'], 0
            blk.indptr, blk.cols = ints.data_ptr(), ints.data_ptr() + 4 * (N + 1)
            blk.adj_ws, blk.adj_ws_bytes = ws.data_ptr(), need
        tar = a['tar']
        blk.tar, blk.tar_stride, blk.B, blk.tar_is64 = tar.data_ptr(), max(B, 1), B, int(tar.dtype == torch.int64)
        blk.last_update, blk.edge_time = _native.ptr(a['lu']), _native.ptr(a['et'])
        blk.last = last.data_ptr()
        blk.xs, blk.h, blk.ldxs, blk.ldh = xs.data_ptr(), h.data_ptr(), ldxs, ldh
        if mlp:
            out = torch.empty((B, self.out_channels), dtype=torch.float32, device=dev)
            blk.out = out.data_ptr()
            _native.check(lib.tgmx_ncn_forward(ctypes.byref(blk), _native.stream_ptr()), 'tgmx_ncn_forward')
            return xs[: B * ldxs].view(B, ldxs), out
        if adj is None:
            _native.check(lib.tgmx_ncn_adj_build(blk.edge_index, blk.ei_is64, blk.ei_stride, E, N, blk.indptr, blk.cols, blk.adj_ws, need,
                                                 _native.stream_ptr()), 'tgmx_ncn_adj_build')  # fmt: skip
        _native.check(lib.tgmx_ncn_cn_emb(blk.x, N, C, self.k, blk.indptr, blk.cols, blk.tar, blk.tar_is64, blk.tar_stride, B, blk.last_update if self.cn_time_decay else 0,
                                          blk.edge_time if self.cn_time_decay else 0, 0 if blk.dup_all else blk.last, blk.xs, ldxs, _native.stream_ptr()),
                      'tgmx_ncn_cn_emb')  # fmt: skip
        return xs[: B * ldxs].view(B, ldxs), None
