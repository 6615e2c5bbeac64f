"""``TGCN`` -- temporal graph convolutional GRU cell (tgm/nn/encoder/tgcn.py:8-157) on HIP kernels.

Parameter names match the reference / PyG (``conv_{u,r,c}.lin.weight``, ``conv_{u,r,c}.bias``,
``linear_{u,r,c}.{weight,bias}``).  ``GCNConv`` is third-party to the reference (torch_geometric);
it is implemented from its published definition (parity unpinned upstream).  The three graph
convolutions share one dense normalised adjacency and run as two exact-fp32 MFMA GEMMs
(``A_hat @ (X [W_u|W_r|W_c])``); snapshot graphs on this path are small (tgbn-trade: 255 nodes).
With gradients enabled the same arithmetic runs inside ``torch.autograd.Function``s with a hand-written backward
(``nn/_tgcn_train.py``: the reference trains this cell, examples/nodeproppred/tgcn.py:92).
"""
from __future__ import annotations

import ctypes
import math
import os
from types import SimpleNamespace
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from . import _ops
from ._fwd_plumbing import carve_scratch, up4
from ._gcn_sparse_train import check_route, route
from ._paramver import TransientCaches
from ._snapshot import GCNGraph, _edge_weight, _endpoints, _Skipped, csr_scratch_sizes, gcn_csr_buffers, gcn_norm_csr, gcn_propagate

_MAX_DENSE_NODES = 16384  # A_hat is dense: 16384^2 floats = 1 GiB


def _cap_message(N: int) -> str:
    return f"tgm_amd GCNConv builds a dense adjacency; {N} nodes exceed {_MAX_DENSE_NODES} (propagate='sparse' takes any number of nodes)"


def _norm_workspace(E: int, N: int, device) -> Tensor:
    nbytes = _native.load().tgmx_gcn_workspace_bytes(E, N)
    return torch.empty(csr_scratch_sizes(E, N, nbytes, 'GCNConv')[4], dtype=torch.int32, device=device)


def _check_graph(module, graph: GCNGraph, edge_weight: Optional[Tensor], N: int) -> None:
    """Host-side checks of a :class:`GCNGraph` handed in place of ``edge_index``."""
    if edge_weight is not None:
        raise ValueError('edge_weight must be None when a GCNGraph is passed: the graph already holds the normalised weights')
    graph.matches(module)
    if graph.num_nodes != N:
        raise ValueError(f'the GCNGraph was built for {graph.num_nodes} nodes, x has {N} rows')


def _graph_for(module, x: Tensor, edge_index, edge_weight: Optional[Tensor]) -> GCNGraph:
    """The caller's :class:`GCNGraph` (checked against the module), or an unbuilt one of this call's own that counts skipped edges into the
    module's counter (``csr`` is ``None``: the caller builds it)."""
    N = x.shape[0]
    if isinstance(edge_index, GCNGraph):
        if edge_index.device != x.device:
            raise ValueError(f'the GCNGraph lives on {edge_index.device}, x on {x.device}')
        return edge_index
    _native.require_device(edge_index, 'edge_index')
    if N == 0:
        raise ValueError('the sparse GCN route needs at least one node')
    E = edge_index.shape[1] if edge_index.dim() == 2 else -1
    return GCNGraph(None, N, E, bool(module.improved), bool(module.add_self_loops), x.device, skipped=module._skipped(x.device), shared=False)


class GCNConv(_Skipped, nn.Module):
    """x' = D^-1/2 (A + I) D^-1/2 x W^T + b  (PyG parameter layout: ``lin.weight`` [out, in], ``bias`` [out]).

    ``propagate='auto'`` (the default): up to ``_MAX_DENSE_NODES`` nodes the adjacency is dense and the propagation a GEMM; above, without
    gradients, it is a CSR by destination and a gather SpMM (``tgmx_gcn_norm_csr`` + ``tgmx_gcn_propagate``; ``check()`` reports edges
    skipped there), and under gradients it raises.  ``'dense'``: the dense path, which raises above the cap.  ``'sparse'``: the CSR route for
    any number of nodes, with and without gradients (``nn/_gcn_sparse_train.py``: nothing ``N x N`` is built or saved).
    ``TGMX_GCN_ROUTE=sparse|dense`` overrides ``'auto'`` only.  A :class:`GCNGraph` (``gcn_graph(...)``) in place of ``edge_index`` selects the
    sparse route and shares one sort among every layer that gets it.  ``cached=True`` is accepted and ignored (the normalisation is
    recomputed per call); to normalise a snapshot once, hand a ``GCNGraph`` in.  The adjacency carries no gradient: edge weights are data."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False, add_self_loops: bool = True,
                 propagate: str = 'auto') -> None:  # fmt: skip
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops = improved, cached, add_self_loops
        self.propagate = check_route(propagate)
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        bound = math.sqrt(6.0 / (self.in_channels + self.out_channels))  # glorot
        nn.init.uniform_(self.lin.weight, -bound, bound)
        nn.init.zeros_(self.bias)

    def _forward_sparse(self, x: Tensor, graph: GCNGraph) -> Tensor:
        """out = A_hat (x W^T) + b over the graph's CSR: one GEMM, one propagate."""
        xw = torch.empty((x.shape[0], self.out_channels), dtype=torch.float32, device=x.device)
        _ops.sgemm_nt(x, self.lin.weight.detach(), xw)
        return gcn_propagate(graph.csr, xw, torch.empty_like(xw), bias=self.bias.detach(), scratch=graph.scratch(self.out_channels), E=graph.E)

    def _sparse(self, x: Tensor, edge_index, edge_weight: Optional[Tensor], grad: bool) -> Tensor:
        graph = _graph_for(self, x, edge_index, edge_weight)
        if graph.csr is None:
            graph.csr = gcn_norm_csr(edge_index, edge_weight, x.shape[0], 2.0 if self.improved else 1.0, self.add_self_loops, graph.skipped,
                                     gcn_csr_buffers(graph.E, x.shape[0], x.device) + [_norm_workspace(graph.E, x.shape[0], x.device)])  # fmt: skip
        if not grad:
            return self._forward_sparse(x, graph)
        from . import _gcn_sparse_train as st

        if st.mode() == 'torch':
            return st.conv_torch(self, graph, x)
        return st.GCNConvSparseFn.apply(self, graph, x, self.lin.weight, self.bias)

    def forward(self, x: Tensor, edge_index: Union[Tensor, GCNGraph], edge_weight: Optional[Tensor] = None) -> Tensor:
        if isinstance(edge_index, GCNGraph):
            _check_graph(self, edge_index, edge_weight, x.shape[0])
        x = _ops._f32c(x, 'x')
        grad = torch.is_grad_enabled() and (x.requires_grad or self.lin.weight.requires_grad or self.bias.requires_grad)
        how = 'sparse' if isinstance(edge_index, GCNGraph) else route(self.propagate)
        if how == 'sparse':
            return self._sparse(x, edge_index, edge_weight, grad)
        if how == 'dense' and x.shape[0] > _MAX_DENSE_NODES:
            raise NotImplementedError(_cap_message(x.shape[0]))
        if x.shape[0] > _MAX_DENSE_NODES and not (
            torch.is_grad_enabled() and (x.requires_grad or self.lin.weight.requires_grad or self.bias.requires_grad)
        ):
            xw = torch.empty((x.shape[0], self.out_channels), dtype=torch.float32, device=x.device)
            _ops.sgemm_nt(x, self.lin.weight.detach(), xw)
            csr = gcn_norm_csr(edge_index, edge_weight, x.shape[0], 2.0 if self.improved else 1.0, self.add_self_loops, self._skipped(x.device))
            return gcn_propagate(csr, xw, torch.empty_like(xw), bias=self.bias.detach())
        A = normalized_adjacency(edge_index, edge_weight, x.shape[0], 2.0 if self.improved else 1.0, self.add_self_loops)
        if torch.is_grad_enabled() and (x.requires_grad or self.lin.weight.requires_grad or self.bias.requires_grad):
            from ._tgcn_train import AdjMatmulFn
            from ._tgn_train import LinearFn

            return AdjMatmulFn.apply(A, LinearFn.apply(x, self.lin.weight, None)) + self.bias
        xwt = torch.empty((self.out_channels, x.shape[0]), dtype=torch.float32, device=x.device)
        _ops.sgemm_nt(self.lin.weight.detach(), x, xwt)  # (X W^T)^T = W X^T
        out = torch.empty((x.shape[0], self.out_channels), dtype=torch.float32, device=x.device)
        return _ops.sgemm_nt(A, xwt, out, bias=self.bias.detach(), K=x.shape[0])


def normalized_adjacency(edge_index: Tensor, edge_weight: Optional[Tensor], N: int, fill: float, add_self_loops: bool) -> Tensor:
    """Dense D^-1/2 (A + I) D^-1/2, rows padded to a multiple of 4 floats (16-byte aligned GEMM operand)."""
    if N > _MAX_DENSE_NODES:
        raise NotImplementedError(_cap_message(N))
    _native.require_device(edge_index, 'edge_index')
    lib = _native.load()
    dev = edge_index.device
    ei = edge_index.to(torch.int64)
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    w = None if edge_weight is None else _ops._f32c(edge_weight, 'edge_weight')
    ld = up4(N)
    A = torch.empty((N, ld), dtype=torch.float32, device=dev)
    ws = torch.empty(2 * N, dtype=torch.float32, device=dev)
    _native.check(
        lib.tgmx_gcn_norm_dense(src.data_ptr(), dst.data_ptr(), _native.ptr(w), src.numel(), N, float(fill), 1 if add_self_loops else 0,
                                A.data_ptr(), ld, ws.data_ptr(), _native.stream_ptr()),
        'tgmx_gcn_norm_dense',
    )  # fmt: skip
    return A[:, :N]


def composed_gcn_conv(conv: GCNConv, x: Tensor, edge_index: Tensor, skipped: Optional[Tensor] = None) -> Tensor:
    """``conv`` (no edge weights) composed from torch ops, device-agnostic and without a data-dependent shape: an edge that is dropped
    (an endpoint out of range; a self loop, which moves to the diagonal) keeps its slot with weight 0."""
    N, E = x.shape[0], edge_index.shape[1]
    src, dst = edge_index[0].long(), edge_index[1].long()
    inside = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    if skipped is not None:
        skipped += (~inside).sum().to(skipped.dtype)
    src, dst = src.clamp(0, max(N - 1, 0)), dst.clamp(0, max(N - 1, 0))
    loop = inside & (src == dst) if conv.add_self_loops else torch.zeros_like(inside)
    w = (inside & ~loop).to(x.dtype)
    # unweighted: an explicit self loop weighs 1 whichever of a node's loops is taken; a node without one gets the fill value
    lw = torch.zeros(N, dtype=x.dtype, device=x.device)
    if conv.add_self_loops:
        has = torch.zeros(N, dtype=x.dtype, device=x.device).index_add_(0, dst, loop.to(x.dtype)) > 0
        lw = torch.where(has, torch.ones_like(lw), torch.full_like(lw, 2.0 if conv.improved else 1.0))
    xw = conv.lin(x)
    if not E:
        dinv = lw.pow(-0.5)
        dinv = dinv.masked_fill(dinv == float('inf'), 0)
        return (dinv * lw * dinv).unsqueeze(1) * xw + conv.bias
    # no float atomics here either (a seeded call repeats bit for bit): the edges in a stable order by destination, one sum per segment
    dst, order = torch.sort(dst, stable=True)
    src, w = src[order], w[order]
    lengths = torch.zeros(N, dtype=torch.int64, device=x.device).index_add_(0, dst, torch.ones_like(dst))
    deg = lw + torch.segment_reduce(w, 'sum', lengths=lengths, unsafe=True)
    dinv = deg.pow(-0.5)
    dinv = dinv.masked_fill(dinv == float('inf'), 0)
    msg = (dinv[src] * w * dinv[dst]).unsqueeze(1) * xw[src]
    out = (dinv * lw * dinv).unsqueeze(1) * xw + torch.segment_reduce(msg, 'sum', lengths=lengths, axis=0, unsafe=True)
    return out + conv.bias


class TGCN(_Skipped, TransientCaches, nn.Module):
    """The TGCN cell.  ``propagate``: ``'auto'`` (the default) is the dense adjacency up to ``_MAX_DENSE_NODES`` nodes; above, it runs the
    sparse route without gradients and raises under them.  ``'dense'`` raises above the cap; ``'sparse'`` is the CSR route for any number
    of nodes, with and without gradients (``tgmx_tgcn_forward_csr`` / ``tgmx_tgcn_backward_csr``: one native call per direction).
    ``TGMX_GCN_ROUTE=sparse|dense`` overrides ``'auto'`` only; a :class:`GCNGraph` in place of ``edge_index`` selects the sparse route.
    ``cached=True`` is accepted and ignored; to normalise a snapshot once, hand a ``GCNGraph`` in.  ``check()`` reports edges the sparse
    route skipped.  The adjacency carries no gradient: edge weights are data."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False, add_self_loops: bool = True,
                 propagate: str = 'auto') -> None:  # fmt: skip
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops = improved, cached, add_self_loops
        self.propagate = check_route(propagate)
        mk = lambda: GCNConv(in_channels, out_channels, improved=improved, cached=cached, add_self_loops=add_self_loops)
        self.conv_c, self.linear_c = mk(), nn.Linear(2 * out_channels, out_channels)
        self.conv_r, self.linear_r = mk(), nn.Linear(2 * out_channels, out_channels)
        self.conv_u, self.linear_u = mk(), nn.Linear(2 * out_channels, out_channels)

    def _stacked(self) -> tuple:
        """(W3 [3C, in], b3 [3C], the three Linear weights, their biases), cached against the parameters' versions."""
        from ._paramver import param_key

        d = self.__dict__
        key = param_key(self)
        if d.get('_tgmx_w3_key') != key:
            convs, lins = (self.conv_u, self.conv_r, self.conv_c), (self.linear_u, self.linear_r, self.linear_c)
            d['_tgmx_w3'] = (torch.cat([c.lin.weight.detach() for c in convs]).contiguous(), torch.cat([c.bias.detach() for c in convs]).contiguous(),
                             [_ops._f32c(l.weight.detach(), 'weight') for l in lins], [_ops._f32c(l.bias.detach(), 'bias') for l in lins])
            d['_tgmx_w3_key'] = key
        return d['_tgmx_w3']

    def _stacked_t(self) -> SimpleNamespace:
        """The transposed weights the sparse backward reads (W3^T [in, 3C], linear_g.weight^T [2C, C]), cached the same way."""
        from ._gcn_sparse_train import cached

        def build() -> SimpleNamespace:
            W3, _, lw, _ = self._stacked()
            return SimpleNamespace(W3T=W3.t().contiguous(), lin_wT=[w.t().contiguous() for w in lw])

        return cached(self, '_tgmx_w3t', build)

    def _forward_sparse(self, x: Tensor, graph: GCNGraph, edges: Optional[tuple], H: Tensor, save: bool = False) -> Tuple[Tensor, Optional[SimpleNamespace]]:
        """The forward over the CSR as ONE native call (``tgmx_tgcn_forward_csr``).  ``edges``: (src, dst, w) of a graph that is not built yet
        -- the call normalises it into the graph's buffers.  ``save``: the saving form (the cat / pre buffers belong to the call)."""
        lib = _native.load()
        N, C, dev = x.shape[0], self.out_channels, x.device
        E = graph.E
        W3, b3, lw, lb = self._stacked()
        nprop = lib.tgmx_cheb_propagate_scratch_floats(E, 3 * C)
        norm_words = 0 if graph.csr is not None else csr_scratch_sizes(E, N, lib.tgmx_gcn_workspace_bytes(E, N), 'TGCN')[4]
        sizes = [3 * C * N, 3 * C * N, norm_words, nprop] + ([] if save else [2 * C * N, C * N, C * N, C * N])
        bufs = carve_scratch(self, sizes, dev)
        if save:
            flat = torch.empty(N * 9 * C, dtype=torch.float32, device=dev)
            parts = flat.split([2 * C * N] * 3 + [C * N] * 3)
            cat, pre = [p.view(N, 2 * C) for p in parts[:3]], [p.view(N, C) for p in parts[3:]]
        else:
            cat, pre = [bufs[4]] * 3, list(bufs[5:8])
        out = torch.empty((N, C), dtype=torch.float32, device=dev)
        a = self.__dict__.get('_tgmx_csr_args')
        if a is None:
            a = self.__dict__['_tgmx_csr_args'] = _native.TgcnCsrFwd()
        a.x, a.ldx, a.N, a.in_ch, a.C = x.data_ptr(), x.stride(0), N, x.shape[1], C
        a.E, a.fill, a.add_self_loops, a.save = E, (2.0 if self.improved else 1.0), (1 if self.add_self_loops else 0), (1 if save else 0)
        if graph.csr is None:
            src, dst, w = edges
            csr = gcn_csr_buffers(E, N, dev)
            a.src, a.dst, a.edge_w, a.idx64, a.csr_built = src.data_ptr(), dst.data_ptr(), _native.ptr(w), int(src.dtype == torch.int64), 0
            a.norm_ws, a.norm_ws_bytes, a.skipped = bufs[2].data_ptr(), bufs[2].numel() * 4, graph.skipped.data_ptr()
        else:
            csr = graph.csr
            a.src = a.dst = a.edge_w = a.norm_ws = a.skipped = None
            a.idx64, a.csr_built, a.norm_ws_bytes = 0, 1, 0
        a.indptr, a.cols, a.vals, a.diag = (t.data_ptr() for t in csr)
        a.W3, a.ldw3, a.b3 = W3.data_ptr(), W3.stride(0), b3.data_ptr()
        for g in range(3):
            a.lin_w[g], a.lin_b[g], a.cat[g], a.pre[g] = lw[g].data_ptr(), lb[g].data_ptr(), cat[g].data_ptr(), pre[g].data_ptr()
        a.H = H.data_ptr()
        a.prop_ws, a.prop_ws_floats = (bufs[3].data_ptr(), nprop) if nprop else (None, 0)
        a.xw, a.G, a.out = bufs[0].data_ptr(), bufs[1].data_ptr(), out.data_ptr()
        _native.check(lib.tgmx_tgcn_forward_csr(ctypes.byref(a), _native.stream_ptr()), 'tgmx_tgcn_forward_csr')
        graph.csr = tuple(csr)
        return out, (SimpleNamespace(cat=cat, pre=pre) if save else None)

    def _sparse(self, x: Tensor, edge_index, edge_weight: Optional[Tensor], H: Tensor, grad: bool) -> Tensor:
        graph = _graph_for(self, x, edge_index, edge_weight)
        edges = None
        if graph.csr is None:
            src, dst = _endpoints(edge_index)
            edges = (src, dst, _edge_weight(edge_weight, src.numel()))
        if not grad:
            return self._forward_sparse(x, graph, edges, H)[0]
        from . import _gcn_sparse_train as st

        if st.mode() == 'torch':
            if graph.csr is None:
                graph.csr = gcn_norm_csr(edge_index, edge_weight, x.shape[0], 2.0 if self.improved else 1.0, self.add_self_loops, graph.skipped,
                                         gcn_csr_buffers(graph.E, x.shape[0], x.device) + [_norm_workspace(graph.E, x.shape[0], x.device)])  # fmt: skip
            return st.cell_torch(self, graph, x, H)
        convs, lins = (self.conv_u, self.conv_r, self.conv_c), (self.linear_u, self.linear_r, self.linear_c)
        return st.TGCNCellSparseFn.apply(self, graph, edges, x, H, *[c.lin.weight for c in convs], *[c.bias for c in convs], *[l.weight for l in lins],
                                         *[l.bias for l in lins])  # fmt: skip

    def forward(self, node_x: Tensor, edge_index: Union[Tensor, GCNGraph], edge_weight: Optional[Tensor] = None, H: Optional[Tensor] = None) -> Tensor:
        if isinstance(edge_index, GCNGraph):
            _check_graph(self, edge_index, edge_weight, node_x.shape[0])
        lib = _native.load()
        x = _ops._f32c(node_x, 'node_x')
        N, C, dev = x.shape[0], self.out_channels, x.device
        f32 = dict(dtype=torch.float32, device=dev)
        H = torch.zeros((N, C), **f32) if H is None else _ops._f32c(H, 'H')
        stream = _native.stream_ptr()
        grad = torch.is_grad_enabled() and (x.requires_grad or H.requires_grad or any(p.requires_grad for p in self.parameters()))
        how = 'sparse' if isinstance(edge_index, GCNGraph) else route(self.propagate)
        if how == 'auto' and not grad and N > _MAX_DENSE_NODES:
            how = 'sparse'  # as GCNConv does there
        if how == 'sparse':
            return self._sparse(x, edge_index, edge_weight, H, grad)
        if not grad and os.environ.get('TGMX_TGCN_PY') is None:
            return self._forward_native(x, edge_index, edge_weight, H)
        A = normalized_adjacency(edge_index, edge_weight, N, 2.0 if self.improved else 1.0, self.add_self_loops)
        if grad:
            from ._tgcn_train import TGCNCellFn

            gates = (self.conv_u, self.conv_r, self.conv_c), (self.linear_u, self.linear_r, self.linear_c)
            return TGCNCellFn.apply(x, A, H, *[c.lin.weight for c in gates[0]], *[c.bias for c in gates[0]], *[l.weight for l in gates[1]],
                                    *[l.bias for l in gates[1]])  # fmt: skip
        # (TGMX_TGCN_PY=1, A/B: the same launches composed from Python, one ctypes call each)
        # the three convolutions share A_hat: G = A_hat @ (X [W_u | W_r | W_c]^T) + [b_u | b_r | b_c]
        W3 = torch.cat([self.conv_u.lin.weight.detach(), self.conv_r.lin.weight.detach(), self.conv_c.lin.weight.detach()])
        b3 = torch.cat([self.conv_u.bias.detach(), self.conv_r.bias.detach(), self.conv_c.bias.detach()])
        xwt = torch.empty((3 * C, N), **f32)
        _ops.sgemm_nt(W3, x, xwt)
        G = torch.empty((N, 3 * C), **f32)
        _ops.sgemm_nt(A, xwt, G, bias=b3, K=N)
        cat = torch.empty((N, 2 * C), **f32)
        pre = [torch.empty((N, C), **f32) for _ in range(3)]  # u, r, c pre-activations
        for g, (lin, gate) in enumerate(((self.linear_u, None), (self.linear_r, None), (self.linear_c, pre[1]))):
            _native.check(lib.tgmx_tgcn_concat(G[:, g * C :].data_ptr(), 3 * C, H.data_ptr(), _native.ptr(gate), C, N, cat.data_ptr(), stream), 'tgmx_tgcn_concat')
            _ops.sgemm_nt(cat, lin.weight.detach(), pre[g], bias=lin.bias.detach())
        out = torch.empty((N, C), **f32)
        _native.check(lib.tgmx_tgcn_output(pre[0].data_ptr(), pre[2].data_ptr(), H.data_ptr(), N * C, out.data_ptr(), stream), 'tgmx_tgcn_output')
        return out

    def _forward_native(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], H: Tensor) -> Tensor:
        """The inference forward as ONE native call (``tgmx_tgcn_forward``): the launches of the Python-composed sequence above in the same order
        (identical results), the stacked GCN weights cached against the parameters' versions, the scratch kept between snapshots -- a
        255-node snapshot is 13 launches and was host-bound at ~160 us when every launch was its own ctypes call between torch ops."""
        if x.shape[0] > _MAX_DENSE_NODES:
            raise NotImplementedError(_cap_message(x.shape[0]))
        _native.require_device(edge_index, 'edge_index')
        lib = _native.load()
        N, C, dev = x.shape[0], self.out_channels, x.device
        d = self.__dict__
        W3, b3, lw, lb = self._stacked()
        ld = up4(N)
        bufs = carve_scratch(self, [N * ld, 2 * N, 3 * C * N, 3 * C * N, 2 * C * N, C * N, C * N, C * N], dev)  # A, norm_ws, xwt, G, cat, pre[0..2]
        ei = edge_index if edge_index.dtype in (torch.int64, torch.int32) else edge_index.to(torch.int64)
        src, dst = ei[0], ei[1]
        if not src.is_contiguous():
            src = src.contiguous()
        if not dst.is_contiguous():
            dst = dst.contiguous()
        w = None if edge_weight is None else _ops._f32c(edge_weight, 'edge_weight')
        out = torch.empty((N, C), dtype=torch.float32, device=dev)
        a = d.get('_tgmx_args')
        if a is None:
            a = d['_tgmx_args'] = _native.TgcnFwd()
        a.x, a.N, a.in_ch, a.C = x.data_ptr(), N, x.shape[1], C
        a.src, a.dst, a.edge_w, a.E = src.data_ptr(), dst.data_ptr(), _native.ptr(w), src.numel()
        a.idx32 = 1 if ei.dtype == torch.int32 else 0
        a.fill, a.add_self_loops = (2.0 if self.improved else 1.0), (1 if self.add_self_loops else 0)
        a.W3, a.b3 = W3.data_ptr(), b3.data_ptr()
        for g in range(3):
            a.lin_w[g], a.lin_b[g] = lw[g].data_ptr(), lb[g].data_ptr()
        a.H = H.data_ptr()
        a.ldA = ld
        a.A, a.norm_ws, a.xwt, a.G, a.cat = (b.data_ptr() for b in bufs[:5])
        for g in range(3):
            a.pre[g] = bufs[5 + g].data_ptr()
        a.out = out.data_ptr()
        _native.check(lib.tgmx_tgcn_forward(ctypes.byref(a), _native.stream_ptr()), 'tgmx_tgcn_forward')
        return out
