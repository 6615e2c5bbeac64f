"""``NCNPredictor`` (tgm/nn/decoder/ncnpred.py; TNCN, https://arxiv.org/abs/2406.07926) -- same constructor arguments, errors, parameter
names, shapes and initialisation order (``xslin.*``, ``xsmlp.{0,2}.*``): a checkpoint of the reference's example loads with
``strict=True``, and back.

``forward(x, edge_index, tar_ei, last_update=None, edge_time=None) -> [B * out_channels]``.  With A the symmetric adjacency of the batch's
sampled subgraph (``A[a, b]`` = how often ``(a, b)`` or ``(b, a)`` occurs in ``edge_index``; a self-loop counts twice), ``R_i[r] = A[tar_i[r]]``,
``I_i[r]`` the ``tar_i[r]``-th unit row, and ``W[r, n] = exp(-(float32(edge_time[r] - last_update[n]) / 10000))`` (1 without
``cn_time_decay``):

    k = 2:  xs = [x[tar_i] * x[tar_j] | ((R_i o R_j) o W) x]
    k = 4:  xs = [x[tar_i] * x[tar_j] | ((I_i o R_j) o W) x | ((R_i o I_j) o W) x | ((R_i o R_j) o W) x]
    k = 8:  with A2 = A A, K3 = A2 A, S_i[r] = A2[tar_i[r]] (kept as R_i is), u[r] = -A[tar_i[r], tar_j[r]] where both sides keep row r (else 0):
            c01 = I_i o R_j    c10 = R_i o I_j    c11 = R_i o R_j    sp = c11 A
            c12 = R_i o S_j + R_i o R_i u         c21 = S_i o R_j + R_j o R_j u
            c22 = S_i o S_j + ([R_i > 0] K3[tar_i, tar_i] + [R_j > 0] K3[tar_j, tar_j] - c11) u + sp
            c12, c21, c22: columns tar_i[r] and tar_j[r] of row r set to 0, then c22 = max(c22, 0)
            xs = [x[tar_i] * x[tar_j] | (c01 o W) x | (c10 o W) x | (c11 o W) x | (c12 o W) x | (c21 o W) x | (c22 o W) x | sp x]
            (sp carries no decay and no column mask; every block is zero unless both sides keep row r)
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

Training (autograd has something to track) is native too at k = 2 / 4: ``forward`` is the same ``tgmx_ncn_forward`` call, writing what the backward
reads into buffers of the call (so the result is the no-grad call's bit for bit, and the positives' and negatives' calls of one step do
not share them), and the backward is ONE native call, ``tgmx_ncn_backward`` (``_ncn_train.py``, ``csrc/ncn_bwd.hip``): the two Linear layers
from the shared blocks, then ``dx`` node by node through two inverted indexes of the pairs and the forward's adjacency -- fixed summation
order, no float atomics, no ``[B, N]`` intermediates.  ``last_update`` / ``edge_time`` get no gradient (the decay weight depends on integers
only) and ``xslin`` gets ``None``.  Outside that path -- autocast, parameters of another dtype, ``get_cn_emb`` under gradients,
``TGMX_NCN_BWD=torch`` -- the same arithmetic is composed from torch ops on the device under autograd, through dense ``[B, N]`` rows (never
``[N, N]``).  ``TGMX_NCN_BWD=py`` issues the native backward's launches one ctypes call each (the same bits).

``k = 8`` (two-hop common neighbours) has its own native stage, ``tgmx_ncn8_forward`` (``csrc/ncn8.hip``): one workgroup per pair expands the
two targets' neighbours' rows into integer count rows (in LDS up to 7680 local ids, in a workspace above), forms every coefficient as an
exact integer and gather-sums ``x`` over ascending ids in float64, rounded once -- nothing ``[N, N]``, no ``[B, N]`` float matrix, the same
bits every run; the two Linear layers, whose 8 C inputs carry those integer weights, run in float64 too (one kernel, rounded once; ``hidden_dim`` up to 8192, a wider layer is an error).  Inference takes it; with gradients k = 8 is the composed torch path (``[B, N]`` rows and ``index_add_`` over the half-edges;
the coefficients carry no gradient), a native k = 8 backward does not exist yet.  One behaviour of the reference is NOT reproduced at k = 8:
it multiplies dense coefficient matrices by ``W``, so a weight that overflows to ``inf`` (``edge_time - last_update`` below about -8.8e5)
turns the zero counts of that row into NaN; here ``W`` multiplies only non-zero counts, as at k = 2 / 4.  On host tensors k = 8 raises
``NotImplementedError`` (device only); k = 2 / 4 raise ``NativeLibraryError`` there.  A pair with a target id outside ``[0, N)`` gives a zero
row, and no gradient, on every path.
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

    Args (the reference's): in_channels, hidden_dim, out_channels, k (2 / 4 / 8: the hops of common-neighbour extraction; 8 adds the
    two-hop blocks), cn_time_decay.  ``duplicate_targets``: ``'last'`` (the reference's CPU behaviour) or ``'all'``.
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
        if self.k == 8 and x.device.type != 'cuda':
            raise NotImplementedError(f'tgm_amd NCNPredictor: k = 8 runs on device tensors only (x lives on {x.device})')
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

        def rows_of(t: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
            keep = ok
            if self.duplicate_targets == 'last':
                last = torch.full((N,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, t, torch.where(ok, ar, -1), 'amax')
                keep = ok & (last[t] == ar)
            R = torch.zeros((B, N), dtype=torch.float32, device=dev)
            if hrow.numel():
                R.index_add_(1, hcol, (hrow[None, :] == t[:, None]).float())  # [B, 2 E] -> [B, N]: counts, exact in float32
            I = torch.zeros((B, N), dtype=torch.float32, device=dev)
            I[ar, t] = 1.0
            return R * keep[:, None], I * keep[:, None], keep

        Ri, Ii, ki = rows_of(ti)
        Rj, Ij, kj = rows_of(tj)
        W = torch.exp(-((a['et'][:, None] - a['lu'][None, :]).to(torch.float32) / 10000)) if self.cn_time_decay else None
        xij = x[ti] * x[tj] * ok[:, None]
        if self.k == 8:
            return torch.cat([xij] + self._torch_cn8(x, ti, tj, ki & kj, Ri, Rj, Ii, Ij, W, hrow, hcol), dim=-1)
        blocks = [(Ri * Rj)] if self.k == 2 else [Ii * Rj, Ri * Ij, Ri * Rj]
        cn = [(b * W if W is not None else b) @ x for b in blocks]
        return torch.cat([xij] + cn, dim=-1)

    @staticmethod
    def _torch_cn8(x: Tensor, ti: Tensor, tj: Tensor, both: Tensor, Ri: Tensor, Rj: Tensor, Ii: Tensor, Ij: Tensor, W: Optional[Tensor], hrow: Tensor,
                   hcol: Tensor) -> list:  # fmt: skip
        """The seven k = 8 blocks from [B, N] rows of exact float32 counts (never [N, N]); only ``... @ x`` carries a gradient."""
        B, N = Ri.shape
        ar = torch.arange(B, device=x.device)

        def hop(M: Tensor) -> Tensor:  # M A: every half-edge (a -> b) adds column a of M onto column b (a slot behind the last row: column N, zeros)
            out = torch.zeros_like(M)
            if hrow.numel():
                out.index_add_(1, hcol, torch.cat([M, M.new_zeros((B, 1))], dim=1)[:, hrow])
            return out

        Si, Sj = hop(Ri), hop(Rj)
        u = -(Ri[ar, tj] * both)[:, None]
        k3i, k3j = (Ri * Si).sum(dim=1, keepdim=True), (Rj * Sj).sum(dim=1, keepdim=True)  # K3[t, t] = sum over m of A[t, m] A2[t, m]
        c11 = Ri * Rj
        sp = hop(c11)
        cols = torch.ones_like(Ri)  # the column masks: tar_i[r] and tar_j[r] of row r
        cols[ar, ti] = 0.0
        cols[ar, tj] = 0.0
        c12 = (Ri * Sj + Ri * Ri * u) * cols
        c21 = (Si * Rj + Rj * Rj * u) * cols
        c22 = ((Si * Sj + ((Ri > 0) * k3i + (Rj > 0) * k3j - c11) * u + sp) * cols).clamp(min=0.0)
        # W multiplies only non-zero counts, as on the native path (an infinite weight leaves the zeros alone)
        wt = (lambda b: b) if W is None else (lambda b: torch.where(b != 0, b * W, b))
        return [wt(b) @ x for b in (Ii * Rj, Ri * Ij, c11, c12, c21, c22)] + [sp @ x]

    # -- inference ------------------------------------------------------------------------------------------------------------------------
    def _weights(self) -> tuple:
        def build(f32) -> '_native.NCNFwd':
            blk = _native.NCNFwd()
            m = self.xsmlp
            blk.w1, blk.b1, blk.w2, blk.b2 = f32(m[0].weight), f32(m[0].bias), f32(m[2].weight), f32(m[2].bias)
            blk.C, blk.k, blk.H, blk.out_ch = self.in_channels, self.k, self.hidden_dim, self.out_channels
            return blk

        return cached_block(self, build)

    def _native_xs(self, a: dict, mlp: bool, force_workspace: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
        """(xs [B, ldxs] scratch view, out [B, out_channels] or None): ``tgmx_ncn_forward`` (k = 8: ``tgmx_ncn8_forward``), or its first two
        stages for ``get_cn_emb``.  ``force_workspace`` (tests; k = 8 without the MLP): the count rows in the workspace whatever N."""
        blk, _ = self._weights()
        lib = _native.load()
        x, N, B, C = a['x'], a['N'], a['B'], self.in_channels
        dev = x.device
        ldxs, ldh = up4(self.k * C), up4(self.hidden_dim)
        adj = a['adj']
        E = adj.num_edges if adj is not None else a['ei'].shape[1]
        need = 0 if adj is not None else _adj_ws_bytes(E)
        own = 0 if adj is not None else (N + 1) + max(2 * E, 1)
        need8 = 0
        if self.k == 8:
            # host arithmetic only; a few bytes while the count rows fit LDS
            need8 = int(lib.tgmx_ncn8_workspace_bytes(max(N, int(lib.tgmx_ncn8_lds_max_nodes())) + 1 if force_workspace else N, B))
            if need8 == 0:
                raise ValueError(f'NCNPredictor: N = {N}, B = {B} are more than the k = 8 stage indexes (< 2^31)')
        # floats and int32 share the scratch buffer: xs, h, last [2 N], then (without a prepared adjacency) indptr, cols, the sort's workspace,
        # and the k = 8 stage's count rows where they do not fit LDS
        xs, h, last, ints, ws, ws8 = carve_scratch(self, [B * ldxs, B * ldh, 2 * N, own, (need + 3) // 4, (need8 + 3) // 4], dev)
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
            if self.k == 8:
                _native.check(lib.tgmx_ncn8_forward(ctypes.byref(blk), ws8.data_ptr(), need8, _native.stream_ptr()), 'tgmx_ncn8_forward')
            else:
                _native.check(lib.tgmx_ncn_forward(ctypes.byref(blk), _native.stream_ptr()), 'tgmx_ncn_forward')
            return xs[: B * ldxs].view(B, ldxs), out
        if adj is None:
            _native.check(lib.tgmx_ncn_adj_build(blk.edge_index, blk.ei_is64, blk.ei_stride, E, N, blk.indptr, blk.cols, blk.adj_ws, need,
                                                 _native.stream_ptr()), 'tgmx_ncn_adj_build')  # fmt: skip
        if self.k == 8:
            _native.check(lib.tgmx_ncn8_cn_emb(blk.x, N, C, blk.indptr, blk.cols, blk.tar, blk.tar_is64, blk.tar_stride, B, blk.last_update if self.cn_time_decay else 0,
                                               blk.edge_time if self.cn_time_decay else 0, 0 if blk.dup_all else blk.last, blk.xs, ldxs, ws8.data_ptr(), need8,
                                               int(force_workspace), _native.stream_ptr()), 'tgmx_ncn8_cn_emb')  # fmt: skip
            return xs[: B * ldxs].view(B, ldxs), None
        _native.check(lib.tgmx_ncn_cn_emb(blk.x, N, C, self.k, blk.indptr, blk.cols, blk.tar, blk.tar_is64, blk.tar_stride, B, blk.last_update if self.cn_time_decay else 0,
                                          blk.edge_time if self.cn_time_decay else 0, 0 if blk.dup_all else blk.last, blk.xs, ldxs, _native.stream_ptr()),
                      'tgmx_ncn_cn_emb')  # fmt: skip
        return xs[: B * ldxs].view(B, ldxs), None
