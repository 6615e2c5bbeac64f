"""``GCNConv`` and ``TGCN`` over the sparse adjacency (``propagate='sparse'``, or a :class:`GCNGraph` handed in), training included.

Forward: ``GCNConv`` is ``tgmx_sgemm_nt`` + ``tgmx_gcn_propagate`` over the CSR by destination; the cell is ONE native call
(``tgmx_tgcn_forward_csr``: normalisation, ``X [W_u|W_r|W_c]^T`` as ``[N, 3C]``, one propagate with the stacked bias, the gates).  Under
gradients the same calls run inside ``torch.autograd.Function``s -- the cell in its saving form, which keeps every gate's ``cat`` and
``pre`` in tensors that belong to the call -- so the grad-enabled forward returns the bits of the no-grad one.

Backward: ONE native call each (``tgmx_gcn_conv_backward_csr``, ``tgmx_tgcn_backward_csr``; ``csrc/gcn_bwd.hip``):

    GCNConv   d b = colsum(dout);  dY = A_hat^T dout;  d W = dY^T x;  d x = dY W
    TGCN      the gate backward, d cat_g = d pre_g W_g with the two reset-gate launches in between, d linear_g.{weight, bias},
              dG = the left halves side by side, d b3 = colsum(dG), dY = A_hat^T dG (one propagate over 3C columns),
              d W3 = dY^T x (rows of gate g: conv_g.lin.weight's gradient), d x = dY W3, d H

``A_hat^T`` is ``tgmx_csr_transpose`` of the forward's CSR (values copied, one sort, no float atomics: two runs give the same bits).  A
module that built the CSR itself from ``edge_index`` saves the CSR and lets the backward call transpose it into its workspace; a
:class:`GCNGraph` builds the transpose once, on first use, and every layer and snapshot that shares the graph hands it in.

``TGMX_TGCN_BWD=py`` issues the same launches one ctypes call each (:func:`conv_backward_per_launch`, :func:`cell_backward_per_launch`: the
readable specification, the same bits); ``TGMX_TGCN_BWD=torch`` runs the layer composed from torch ops under autograd (``index_add`` over
the CSR's entries).  What is saved: the CSR (or the graph), ``x``, ``H``, the ``cat`` / ``pre`` buffers and the weights -- nothing ``N x N``.
The adjacency carries no gradient: edge weights are data, as on the dense path.
"""
from __future__ import annotations

import ctypes
import os

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _native
from ._fwd_plumbing import up4
from ._paramver import param_key
from ._snapshot import GCNGraph

ROUTES = ('auto', 'dense', 'sparse')


def check_route(propagate: str) -> str:
    if propagate not in ROUTES:
        raise ValueError(f"propagate must be one of {ROUTES}, got {propagate!r}")
    return propagate


def route(propagate: str) -> str:
    """The module's route: its ``propagate=``, with ``TGMX_GCN_ROUTE=sparse|dense`` overriding ``'auto'`` only."""
    if propagate == 'auto':
        env = os.environ.get('TGMX_GCN_ROUTE', '')
        if env in ('sparse', 'dense'):
            return env
    return propagate


def mode() -> str:
    """'native' (default), 'py' or 'torch': ``TGMX_TGCN_BWD``."""
    m = os.environ.get('TGMX_TGCN_BWD', '')
    return m if m in ('py', 'torch') else 'native'


def cached(owner, name: str, build):
    """``build()`` of ``owner``'s parameters, cached on ``owner`` against their versions."""
    d, key = owner.__dict__, param_key(owner)
    if d.get(name + '_key') != key:
        d[name], d[name + '_key'] = build(), key
    return d[name]


def _csr_ptrs(t, graph: GCNGraph, want_t: bool) -> list:
    """Fill the CSR fields of an argument block; returns what must stay alive.  A shared graph hands its transpose in (built once)."""
    indptr, cols, vals, diag = graph.csr
    t.indptr, t.cols, t.vals, t.diag, t.nnz = indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), graph.E
    if want_t and graph.shared:
        it, ct, vt, _ = graph.transposed()
        t.indptr_t, t.cols_t, t.vals_t = it.data_ptr(), ct.data_ptr(), vt.data_ptr()
        return [it, ct, vt]
    t.indptr_t = t.cols_t = t.vals_t = None
    return []


def _run(t, dev, name: str, per_launch) -> None:
    """The backward over the filled block ``t``: the one call, or its launches one by one."""
    if mode() == 'py':
        per_launch(t, dev)
        return
    lib = _native.load()
    need = int(getattr(lib, name + '_workspace_bytes')(ctypes.byref(t)))
    if need == 0:
        _native.check(-1, name + '_workspace_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need
    _native.check(getattr(lib, name)(ctypes.byref(t), _native.stream_ptr()), name)
    t.workspace, t.workspace_bytes = None, 0


def _contig(g: Tensor) -> Tensor:
    g = g if g.dtype == torch.float32 else g.float()
    return g if g.is_contiguous() else g.contiguous()


# ---- GCNConv ------------------------------------------------------------------------------------------------------------------------------
class GCNConvSparseFn(torch.autograd.Function):
    """out = A_hat (x W^T) + b over ``graph``'s CSR.  Inputs after the module and the graph: x, lin.weight, bias."""

    @staticmethod
    def forward(ctx, conv, graph: GCNGraph, x: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
        out = conv._forward_sparse(x, graph)
        ctx.conv, ctx.graph = conv, graph
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout: Tensor):
        conv, graph = ctx.conv, ctx.graph
        x, W = ctx.saved_tensors
        need = ctx.needs_input_grad
        N, cin, C, dev = x.shape[0], x.shape[1], W.shape[0], x.device
        dout = _contig(dout)
        t = _native.GcnConvBwd()
        t.N, t.in_ch, t.C = N, cin, C
        t.x, t.ldx, t.dout, t.lddo = x.data_ptr(), x.stride(0), dout.data_ptr(), dout.stride(0)
        keep = _csr_ptrs(t, graph, need[2] or need[3])
        dW = torch.empty((C, cin), dtype=torch.float32, device=dev) if need[3] else None
        db = torch.empty(C, dtype=torch.float32, device=dev) if need[4] else None
        dx = torch.empty((N, cin), dtype=torch.float32, device=dev) if need[2] else None
        if need[2]:
            WT = cached(conv, '_tgmx_wt', lambda: conv.lin.weight.detach().t().contiguous())
            t.WT, t.ldwt = WT.data_ptr(), C
        t.d_W, t.d_b, t.d_x = _native.ptr(dW), _native.ptr(db), _native.ptr(dx)
        _run(t, dev, 'tgmx_gcn_conv_backward_csr', conv_backward_per_launch)
        del keep
        return None, None, dx, dW, db


def _transposed_for(t, N: int, keep: list) -> tuple:
    """(indptr_t, cols_t, vals_t) as device pointers: the block's own, or ``tgmx_csr_transpose`` into fresh tensors."""
    if t.indptr_t:
        return t.indptr_t, t.cols_t, t.vals_t
    lib, dev = _native.load(), keep[0].device
    E = t.nnz
    nbytes = lib.tgmx_csr_transpose_workspace_bytes(E, N)
    if nbytes == 0:
        raise ValueError(f'{E} entries over {N} nodes are out of range')
    keep += [torch.empty(N + 1, dtype=torch.int32, device=dev), torch.empty(max(E, 1), dtype=torch.int32, device=dev),
             torch.empty(max(E, 1), dtype=torch.float32, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)]  # fmt: skip
    it, ct, vt, ws = (k.data_ptr() for k in keep[-4:])
    _native.check(lib.tgmx_csr_transpose(t.indptr, t.cols, t.vals, t.diag, N, E, it, ct, vt, None, ws, nbytes, _native.stream_ptr()), 'tgmx_csr_transpose')
    return it, ct, vt


def _propagate_t(t, csr_t: tuple, N: int, C: int, src: int, lds: int, out: int, ldo: int, keep: list) -> None:
    lib = _native.load()
    nprop = lib.tgmx_cheb_propagate_scratch_floats(t.nnz, C)
    prop = None
    if nprop:
        keep.append(torch.empty(nprop, dtype=torch.float32, device=keep[0].device))
        prop = keep[-1].data_ptr()
    _native.check(lib.tgmx_gcn_propagate(*csr_t, t.diag, N, C, src, lds, None, _native.GCN_EPI['none'], None, 0, 0.0, None, None, 0, out, ldo, t.nnz,
                                         prop, nprop, _native.stream_ptr()), 'tgmx_gcn_propagate')  # fmt: skip


def conv_backward_per_launch(t, dev) -> None:
    """What ``tgmx_gcn_conv_backward_csr`` composes, in its order with its kernels; every region of its workspace is a tensor here."""
    lib, st = _native.load(), _native.stream_ptr()
    N, C, cin = t.N, t.C, t.in_ch
    keep: list = [torch.empty(1, device=dev)]

    def buf(n: int) -> int:
        keep.append(torch.empty(max(1, n), dtype=torch.float32, device=dev))
        return keep[-1].data_ptr()

    if t.d_b:
        _native.check(lib.tgmx_colsum(t.dout, t.lddo, N, C, t.d_b, 0, buf(256 * C), st), 'tgmx_colsum')
    if t.d_W or t.d_x:
        csr_t = _transposed_for(t, N, keep)
        ldy = up4(C)
        dY = buf(N * ldy)
        _propagate_t(t, csr_t, N, C, t.dout, t.lddo, dY, ldy, keep)
        if t.d_W:
            part = buf(lib.tgmx_sgemm_tn_workspace_bytes(N, C, cin, 1) // 4 + 1)
            _native.check(lib.tgmx_sgemm_tn(dY, ldy, t.x, t.ldx, t.d_W, cin, N, C, cin, 1, 0, 0, 0, 0, part, st), 'tgmx_sgemm_tn')
        if t.d_x:
            _native.check(lib.tgmx_sgemm_nt(dY, ldy, t.WT, t.ldwt, t.d_x, cin, N, cin, C, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')


# ---- the TGCN cell ------------------------------------------------------------------------------------------------------------------------
class TGCNCellSparseFn(torch.autograd.Function):
    """The whole cell over ``graph``'s CSR.  Inputs after the module and the graph: x, H, then the parameters in the order
    conv_{u,r,c}.lin.weight, conv_{u,r,c}.bias, linear_{u,r,c}.weight, linear_{u,r,c}.bias."""

    @staticmethod
    def forward(ctx, cell, graph: GCNGraph, edges, x: Tensor, H: Tensor, *params: Tensor) -> Tensor:
        out, s = cell._forward_sparse(x, graph, edges, H, save=True)
        ctx.cell, ctx.graph = cell, graph
        ctx.save_for_backward(x, H, *s.cat, *s.pre)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout: Tensor):
        cell, graph = ctx.cell, ctx.graph
        x, H = ctx.saved_tensors[:2]
        cat, pre = ctx.saved_tensors[2:5], ctx.saved_tensors[5:8]
        need = ctx.needs_input_grad
        N, cin, C, dev = x.shape[0], x.shape[1], cell.out_channels, x.device
        f32 = dict(dtype=torch.float32, device=dev)
        dout = _contig(dout)
        w = cell._stacked_t()
        t = _native.TgcnCsrBwd()
        t.N, t.in_ch, t.C = N, cin, C
        t.x, t.ldx, t.H, t.dout = x.data_ptr(), x.stride(0), H.data_ptr(), dout.data_ptr()
        t.W3T, t.ldw3t = w.W3T.data_ptr(), 3 * C
        for g in range(3):
            t.lin_wT[g], t.cat[g], t.pre[g] = w.lin_wT[g].data_ptr(), cat[g].data_ptr(), pre[g].data_ptr()
        n_cw, n_cb, n_lw, n_lb = need[5:8], need[8:11], need[11:14], need[14:17]
        keep = _csr_ptrs(t, graph, need[3] or any(n_cw))
        dW3 = torch.empty((3 * C, cin), **f32) if any(n_cw) else None
        db3 = torch.empty(3 * C, **f32) if any(n_cb) else None
        d_lw = [torch.empty((C, 2 * C), **f32) if n else None for n in n_lw]
        d_lb = [torch.empty(C, **f32) if n else None for n in n_lb]
        dx = torch.empty((N, cin), **f32) if need[3] else None
        dH = torch.empty((N, C), **f32) if need[4] else None
        t.d_W3, t.d_b3, t.d_x, t.d_H = _native.ptr(dW3), _native.ptr(db3), _native.ptr(dx), _native.ptr(dH)
        for g in range(3):
            t.d_lw[g], t.d_lb[g] = _native.ptr(d_lw[g]), _native.ptr(d_lb[g])
        _run(t, dev, 'tgmx_tgcn_backward_csr', cell_backward_per_launch)
        del keep, w
        d_cw = [dW3[g * C : (g + 1) * C] if n else None for g, n in enumerate(n_cw)]
        d_cb = [db3[g * C : (g + 1) * C] if n else None for g, n in enumerate(n_cb)]
        return (None, None, None, dx, dH, *d_cw, *d_cb, *d_lw, *d_lb)


def cell_backward_per_launch(t, dev) -> None:
    """What ``tgmx_tgcn_backward_csr`` composes, in its order with its kernels; every region of its workspace is a tensor here."""
    lib, st = _native.load(), _native.stream_ptr()
    N, C, cin = t.N, t.C, t.in_ch
    keep: list = [torch.empty(1, device=dev)]

    def buf(n: int) -> int:
        keep.append(torch.empty(max(1, n), dtype=torch.float32, device=dev))
        return keep[-1].data_ptr()

    def nt(A: int, B: int, out: int) -> None:  # d cat_g = d pre_g W_g
        _native.check(lib.tgmx_sgemm_nt(A, C, B, C, out, 2 * C, N, 2 * C, C, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')

    du, dr, dc = buf(N * C), buf(N * C), buf(N * C)
    dcat = [buf(N * 2 * C) for _ in range(3)]
    dH = t.d_H or buf(N * C)
    tn_part = buf(max(lib.tgmx_sgemm_tn_workspace_bytes(N, C, 2 * C, 1), lib.tgmx_sgemm_tn_workspace_bytes(N, 3 * C, cin, 1)) // 4 + 1)
    cs_part = buf(256 * 3 * C)
    _native.check(lib.tgmx_tgcn_gate_backward(t.dout, t.pre[0], t.pre[2], t.H, N * C, du, dc, dH, st), 'tgmx_tgcn_gate_backward')
    nt(du, t.lin_wT[0], dcat[0])
    nt(dc, t.lin_wT[2], dcat[2])
    _native.check(lib.tgmx_tgcn_reset_backward(dcat[2], dcat[0], None, t.pre[1], t.H, C, N, dr, dH, st), 'tgmx_tgcn_reset_backward')
    nt(dr, t.lin_wT[1], dcat[1])
    _native.check(lib.tgmx_tgcn_reset_backward(None, None, dcat[1], None, None, C, N, None, dH, st), 'tgmx_tgcn_reset_backward')
    for g, dpre in enumerate((du, dr, dc)):
        if t.d_lw[g]:
            _native.check(lib.tgmx_sgemm_tn(dpre, C, t.cat[g], 2 * C, t.d_lw[g], 2 * C, N, C, 2 * C, 1, 0, 0, 0, 0, tn_part, st), 'tgmx_sgemm_tn')
        if t.d_lb[g]:
            _native.check(lib.tgmx_colsum(dpre, C, N, C, t.d_lb[g], 0, cs_part, st), 'tgmx_colsum')
    if not (t.d_W3 or t.d_b3 or t.d_x):
        return
    dG = buf(N * 3 * C)  # the left halves of the three d cat side by side
    _native.check(lib.tgmx_tgcn_gather_left(dcat[0], dcat[1], dcat[2], C, N, dG, st), 'tgmx_tgcn_gather_left')
    if t.d_b3:
        _native.check(lib.tgmx_colsum(dG, 3 * C, N, 3 * C, t.d_b3, 0, cs_part, st), 'tgmx_colsum')
    if t.d_W3 or t.d_x:
        csr_t = _transposed_for(t, N, keep)
        ldg = up4(3 * C)
        dY = buf(N * ldg)
        _propagate_t(t, csr_t, N, 3 * C, dG, 3 * C, dY, ldg, keep)
        if t.d_W3:
            _native.check(lib.tgmx_sgemm_tn(dY, ldg, t.x, t.ldx, t.d_W3, cin, N, 3 * C, cin, 1, 0, 0, 0, 0, tn_part, st), 'tgmx_sgemm_tn')
        if t.d_x:
            _native.check(lib.tgmx_sgemm_nt(dY, ldg, t.W3T, t.ldw3t, t.d_x, cin, N, cin, 3 * C, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')


# ---- composed from torch ops (TGMX_TGCN_BWD=torch) ----------------------------------------------------------------------------------------
def adj_matmul_torch(graph: GCNGraph, y: Tensor) -> Tensor:
    """A_hat y from the CSR's entries by ``index_add`` (differentiable in ``y``; reads the entry count back: the A/B path only)."""
    indptr, cols, vals, diag = graph.csr
    nnz = int(indptr[-1])
    rows = torch.repeat_interleave(torch.arange(graph.num_nodes, device=y.device), (indptr[1:] - indptr[:-1]).long())
    return (diag.unsqueeze(1) * y).index_add(0, rows, vals[:nnz].unsqueeze(1) * y[cols[:nnz].long()])


def conv_torch(conv, graph: GCNGraph, x: Tensor) -> Tensor:
    return adj_matmul_torch(graph, conv.lin(x)) + conv.bias


def cell_torch(cell, graph: GCNGraph, x: Tensor, H: Tensor) -> Tensor:
    cu, cr, cc = (conv_torch(c, graph, x) for c in (cell.conv_u, cell.conv_r, cell.conv_c))
    U = torch.sigmoid(cell.linear_u(torch.cat([cu, H], dim=1)))
    R = torch.sigmoid(cell.linear_r(torch.cat([cr, H], dim=1)))
    Ht = torch.tanh(cell.linear_c(torch.cat([cc, H * R], dim=1)))
    return U * H + (1 - U) * Ht


__all__ = ['GCNConvSparseFn', 'TGCNCellSparseFn', 'adj_matmul_torch', 'cell_backward_per_launch', 'cell_torch', 'check_route', 'conv_backward_per_launch',
           'conv_torch', 'mode', 'route']  # fmt: skip
