"""A restatement of GCNConv and the TGCN cell over an EDGE LIST (test infrastructure; imports nothing of the product path).

float64 by default, ``index_add_`` over the edges and never a dense ``N x N``: 20 000 nodes cost nothing.  ``dtype=torch.float32`` gives the
restatement's own rounding error.  Everything is plain torch, so gradients come from autograd (there are no hand-written ones here).

The normalisation is PyG's ``gcn_norm`` with ``add_remaining_self_loops`` as the library states it: an edge with an endpoint outside
``[0, N)`` is dropped; with ``add_self_loops`` a node's loop weight is ``fill`` (1, or 2 for ``improved``) unless it has an explicit self
loop, then that loop's weight (of several, the one at the highest edge position), and explicit loops leave the edge list; the degree is
taken over the destination and includes the loop weight; degree 0 gives the factor 0.  Without ``add_self_loops`` loops are ordinary
edges and the diagonal is 0.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch
from torch import Tensor

F64 = torch.float64


class Graph(NamedTuple):
    src: Tensor  # [nnz] the kept edges, in edge order
    dst: Tensor
    vals: Tensor  # [nnz] dinv[src] w dinv[dst]
    diag: Tensor  # [N]
    N: int


def gcn_norm(edge_index: Tensor, edge_weight: Optional[Tensor], N: int, improved: bool = False, add_self_loops: bool = True, dtype=F64) -> Graph:
    src, dst = edge_index[0].long().cpu(), edge_index[1].long().cpu()
    E = src.numel()
    w_all = torch.ones(E, dtype=dtype) if edge_weight is None else edge_weight.detach().cpu().to(dtype)
    pos = torch.arange(E)
    inside = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    src, dst, w, pos = src[inside], dst[inside], w_all[inside], pos[inside]
    loop_w = torch.zeros(N, dtype=dtype)
    if add_self_loops:
        loop = src == dst
        loop_w = torch.full((N,), 2.0 if improved else 1.0, dtype=dtype)
        last = torch.full((N,), -1, dtype=torch.int64).scatter_reduce(0, dst[loop], pos[loop], 'amax')
        has = last >= 0
        loop_w[has] = w_all[last[has]]
        src, dst, w = src[~loop], dst[~loop], w[~loop]
    deg = loop_w.clone().index_add_(0, dst, w)
    dinv = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    return Graph(src, dst, dinv[src] * w * dinv[dst], dinv * loop_w * dinv, N)


def adj_matmul(g: Graph, y: Tensor, transpose: bool = False) -> Tensor:
    """A_hat y (A_hat[dst, src] = vals), or A_hat^T y."""
    rows, cols = (g.src, g.dst) if transpose else (g.dst, g.src)
    vals, diag = g.vals.to(y.dtype), g.diag.to(y.dtype)
    return (diag.unsqueeze(1) * y).index_add(0, rows, vals.unsqueeze(1) * y[cols])


def adj_abs_matmul(g: Graph, y: Tensor, transpose: bool = False) -> Tensor:
    """sum |v| |y| per output element: the magnitude an error bound for the sum scales with."""
    return adj_matmul(Graph(g.src, g.dst, g.vals.abs(), g.diag.abs(), g.N), y.abs(), transpose)


def row_lengths(g: Graph, transpose: bool = False) -> Tensor:
    return torch.zeros(g.N, dtype=torch.int64).index_add_(0, g.src if transpose else g.dst, torch.ones_like(g.src))


def gcn_conv(g: Graph, x: Tensor, W: Tensor, b: Tensor) -> Tensor:
    return adj_matmul(g, x @ W.T) + b


def tgcn_cell(p: Dict[str, Tensor], g: Graph, x: Tensor, H: Optional[Tensor] = None) -> Tensor:
    C = p['linear_u.weight'].shape[0]
    H = torch.zeros(x.shape[0], C, dtype=x.dtype) if H is None else H
    conv = lambda k: gcn_conv(g, x, p[f'conv_{k}.lin.weight'], p[f'conv_{k}.bias'])
    lin = lambda k, v: v @ p[f'linear_{k}.weight'].T + p[f'linear_{k}.bias']
    U = torch.sigmoid(lin('u', torch.cat([conv('u'), H], 1)))
    R = torch.sigmoid(lin('r', torch.cat([conv('r'), H], 1)))
    Cc = torch.tanh(lin('c', torch.cat([conv('c'), H * R], 1)))
    return U * H + (1 - U) * Cc


def triples(g: Graph):
    """The off-diagonal entries as (row = dst, col = src, value) rows."""
    return g.dst, g.src, g.vals
