"""Training path of ``GCLSTM`` / ``ChebConv`` (tgm/nn/encoder/gclstm.py under ``loss.backward()``, examples/linkproppred/gclstm.py): a
``torch.autograd.Function`` whose forward is the inference call (``tgmx_gclstm_forward``: the same kernels in the same order, so the
grad-enabled forward returns the bits of the no-grad one) and whose backward is ONE native call (``tgmx_gclstm_backward``,
``csrc/cheb_bwd.hip``):

    the gate backward                     -> ``tgmx_gclstm_gate_backward`` (I, F, T, O, C' recomputed from ``pre`` and ``C``)
    d W_g, d conv_g.lins.k.weight         -> two batched ``tgmx_sgemm_tn``, written as [4, in, C] and [K, 4, C, C]: every parameter's
                                             gradient is a contiguous view, no torch transpose or slice copies afterwards
    d b_g, d conv_g.bias                  -> one ``tgmx_colsum`` of ``dpre`` (the second gets a copy: the two must not share memory)
    d node_x, the gradient at the basis   -> ``tgmx_sgemm_nt`` on the transposed stacked weight, only the columns somebody asked for
    d H (K > 1)                           -> ``tgmx_cheb_laplacian_t`` and the reverse recurrence in Clenshaw form
                                             (``tgmx_cheb_clenshaw``: K - 1 ``tgmx_cheb_propagate2`` launches, no axpy)

``TGMX_GCLSTM_BWD=py`` issues the backward's launches one ctypes call each from :func:`backward_per_launch` -- the readable
specification, the same bits; ``TGMX_GCLSTM_BWD=torch`` keeps the composed torch path (the modules then never come here).

What is saved.  ``op = [x | Tx_0 .. Tx_{K-1}]`` and ``pre`` are written by the forward into tensors that belong to THE CALL (a BPTT loop,
or two calls before one ``backward()``, must not overwrite what the first call saved), together with ``C`` (the caller's tensor, saved
through autograd so that an in-place write before ``backward()`` is refused) and the call's edge list (``edge_index`` rows, weights,
``lambda_max``).  The transposed Laplacian is NOT kept: the backward rebuilds it from the saved edge list
with ``tgmx_cheb_laplacian_t`` (one sort; E entries per call would otherwise stay alive for every snapshot of a BPTT window), and only
when ``H`` wants a gradient and K > 1 -- the example's loop (``h_0`` / ``c_0`` detached) never builds it.  The builder shares the
forward's degree, entry and diagonal code, so the rebuilt entries are the forward's bit for bit.  The CSR of the forward, its sort
workspace and the propagate's chunk sums are dead after the forward and stay in the module's shared scratch.  The stacked weight and its
transpose are made once per parameter version (``cached_weights``, one ``tgmx_pack2d``).  ``edge_weight`` and ``lambda_max`` are data: no
gradient, as in ``_tgcn_train.py``.
"""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace
from typing import List, Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _native
from ._fwd_plumbing import up4
from ._paramver import param_key, param_list
from ._snapshot import _edge_weight, _endpoints


def mode() -> str:
    """'native' (default), 'py' or 'torch': ``TGMX_GCLSTM_BWD``."""
    m = os.environ.get('TGMX_GCLSTM_BWD', '')
    return m if m in ('py', 'torch') else 'native'


def in_envelope(module, tensors, edge_weight, lambda_max) -> bool:
    """The native training path takes the call: float32 tensors on one device, no autocast, contiguous float32 parameters there, at least
    one node, and no gradient asked of ``edge_weight`` / ``lambda_max``."""
    if mode() == 'torch' or torch.is_autocast_enabled():
        return False
    dev = tensors[0].device
    if tensors[0].shape[0] == 0 or any(t.device != dev or t.dtype != torch.float32 for t in tensors):
        return False
    if any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in param_list(module)):
        return False
    if edge_weight is not None and edge_weight.requires_grad:
        return False
    return not (isinstance(lambda_max, Tensor) and lambda_max.requires_grad)


def _up64(n: int) -> int:
    return (n + 63) // 64 * 64


def transposed_weight(owner, W: Tensor, rows: int, cols: int) -> Tensor:
    """W[:rows, :cols]^T as [cols, rows] (one ``tgmx_pack2d``), cached on ``owner`` against its parameters' versions."""
    d = owner.__dict__
    key = param_key(owner)
    if d.get('_tgmx_wtkey') != key:
        WT = torch.empty((cols, rows), dtype=torch.float32, device=W.device)
        job = (_native.PackJob * 1)()
        j = job[0]
        j.src, j.dst, j.src_ld, j.dst_ld, j.rows, j.cols, j.dst_rows, j.dst_cols, j.transpose = W.data_ptr(), WT.data_ptr(), W.stride(0), rows, cols, rows, cols, rows, 1
        _native.check(_native.load().tgmx_pack2d(job, 1, _native.stream_ptr()), 'tgmx_pack2d')
        d['_tgmx_wt'], d['_tgmx_wtkey'] = WT, key
    return d['_tgmx_wt']


def _grad_views(shapes, device) -> List[Tensor]:
    """One contiguous float32 tensor per shape, carved from one allocation (each on the 256-byte grid)."""
    sizes = [_up64(int(torch.Size(s).numel())) for s in shapes]
    flat = torch.empty(max(1, sum(sizes)), dtype=torch.float32, device=device)
    return [v[: torch.Size(s).numel()].view(s) for v, s in zip(flat.split(sizes), shapes)]


def _rows(g: Optional[Tensor]) -> Optional[Tensor]:
    """An upstream gradient as float32 rows with unit column stride (``stride(0)`` is the leading dimension)."""
    if g is None:
        return None
    g = g if g.dtype == torch.float32 else g.float()
    return g if (g.stride(1) == 1 and g.stride(0) >= g.shape[1]) else g.contiguous()


def _run(t, dev) -> None:
    """The backward over the filled block ``t``: the one call, or its launches one by one."""
    if mode() == 'py':
        backward_per_launch(t, dev)
        return
    lib = _native.load()
    need = int(lib.tgmx_gclstm_backward_workspace_bytes(ctypes.byref(t)))
    if need == 0:
        _native.check(-1, 'tgmx_gclstm_backward_workspace_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need
    _native.check(lib.tgmx_gclstm_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_gclstm_backward')
    t.workspace, t.workspace_bytes = None, 0


class GclstmFunction(torch.autograd.Function):
    """``tensors``: node_x, H, C (``None`` for a state that starts at zero), then every parameter of the cell in ``parameters()`` order."""

    @staticmethod
    def forward(ctx, cell, edge_index: Tensor, edge_weight: Optional[Tensor], lam: float, lam_t: Optional[Tensor], *tensors):
        node_x, H, C = tensors[:3]
        H_out, C_out, s = cell._forward_native(node_x, edge_index, edge_weight, None if H is None else H.detach(), None if C is None else C.detach(),
                                               lam, lam_t, own=True)  # fmt: skip
        ctx.cell, ctx.s = cell, s
        ctx.save_for_backward(s.C)  # (the caller's own tensor, not a copy: autograd then refuses a backward after an in-place write to it)
        ctx.set_materialize_grads(False)
        return H_out, C_out

    @staticmethod
    @once_differentiable
    def backward(ctx, dH: Optional[Tensor], dC: Optional[Tensor]):
        cell, s = ctx.cell, ctx.s
        need = ctx.needs_input_grad
        params = param_list(cell)
        grads: List[Optional[Tensor]] = [None] * (5 + 3 + len(params))
        if dH is None and dC is None:
            return tuple(grads)
        N, Co, K, cin, dev = s.N, cell.out_channels, cell.K, cell.in_channels, s.op.device
        dH, dC = _rows(dH), _rows(dC)
        slots = {}  # id(parameter) -> (group, index of its view in the group's tensor)
        for g, (Wg, bg, conv) in enumerate(cell._gates()):
            slots[id(Wg)], slots[id(bg)] = ('W', g), ('b', g)
            for k, lin in enumerate(conv.lins):
                slots[id(lin.weight)] = ('lins', (k, g))
            if conv.bias is not None:
                slots[id(conv.bias)] = ('cb', g)
        wanted = {slots[id(p)][0] for p, n in zip(params, need[8:]) if n}
        dW, dL, db, dcb, dx, dHp, dCp = _grad_views([(4, cin, Co), (K, 4, Co, Co), (4, 1, Co), (4, Co), (N, cin), (N, Co), (N, Co)], dev)
        t = _native.GclstmBwd()
        t.N, t.in_ch, t.C, t.K, t.normalization = N, cin, Co, K, _native.CHEB_NORM[cell.normalization]
        (Cprev,) = ctx.saved_tensors
        t.op, t.ldop, t.pre, t.Cprev = s.op.data_ptr(), s.ld, s.pre.data_ptr(), Cprev.data_ptr()
        t.dH_out, t.lddh = _native.ptr(dH), 0 if dH is None else dH.stride(0)
        t.dC_out, t.lddc = _native.ptr(dC), 0 if dC is None else dC.stride(0)
        t.src, t.dst, t.idx64, t.edge_w, t.E, _, t.lambda_max, t.lambda_ptr = _graph_args(s, cell.normalization)
        t.d_W = dW.data_ptr() if 'W' in wanted else None
        t.d_lins = dL.data_ptr() if 'lins' in wanted else None
        t.d_b = db.data_ptr() if 'b' in wanted else None
        t.d_conv_bias = dcb.data_ptr() if 'cb' in wanted else None
        t.d_x = dx.data_ptr() if need[5] else None
        t.d_H = dHp.data_ptr() if need[6] else None
        t.d_Cprev = dCp.data_ptr() if need[7] else None
        if need[5] or need[6]:
            W, _ = cell._stacked(dev)
            WT = transposed_weight(cell, W, 4 * Co, cin + K * Co)
            t.WT, t.ldwt = WT.data_ptr(), 4 * Co
        _run(t, dev)
        grads[5], grads[6], grads[7] = (dx if need[5] else None), (dHp if need[6] else None), (dCp if need[7] else None)
        group = dict(W=dW, lins=dL, b=db, cb=dcb)
        for i, (p, n) in enumerate(zip(params, need[8:])):
            if n:
                kind, ix = slots[id(p)]
                grads[8 + i] = group[kind][ix]
        return tuple(grads)


def apply(cell, node_x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], H: Optional[Tensor], C: Optional[Tensor], lam: float,
          lam_t: Optional[Tensor]):  # fmt: skip
    """The cell's training path: ``(H, C)`` with ``grad_fn`` = :class:`GclstmFunction`."""
    return GclstmFunction.apply(cell, edge_index, edge_weight, lam, lam_t, node_x, H, C, *param_list(cell))


class ChebConvFunction(torch.autograd.Function):
    """``ChebConv`` under gradients from the same pieces: d lins.k.weight = dout^T Tx_k (one batched ``tgmx_sgemm_tn`` into [K, out, in]),
    d bias = the column sums of dout, d x = the Clenshaw pass over dout Wstack.  ``tensors``: x, then the parameters."""

    @staticmethod
    def forward(ctx, conv, edge_index: Tensor, edge_weight: Optional[Tensor], lam: float, lam_t: Optional[Tensor], *tensors):
        out, s = conv._forward_native(tensors[0], edge_index, edge_weight, lam, lam_t, own=True)
        ctx.conv, ctx.s = conv, s
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout: Tensor):
        lib, st = _native.load(), _native.stream_ptr()
        conv, s = ctx.conv, ctx.s
        need = ctx.needs_input_grad
        params = param_list(conv)
        N, K, cin, cout, dev = s.N, len(conv.lins), conv.in_channels, conv.out_channels, s.op.device
        dout = _rows(dout)
        dL, db, dx = _grad_views([(K, cout, cin), (cout,), (N, cin)], dev)
        keep: list = []

        def buf(n: int, dtype=torch.float32) -> int:
            keep.append(torch.empty(max(1, n), dtype=dtype, device=dev))
            return keep[-1].data_ptr()

        weights = {id(lin.weight): k for k, lin in enumerate(conv.lins)}
        if any(n and id(p) in weights for p, n in zip(params, need[6:])):
            part = buf(lib.tgmx_sgemm_tn_workspace_bytes(N, cout, cin, K) // 4)
            _native.check(lib.tgmx_sgemm_tn(dout.data_ptr(), dout.stride(0), s.op.data_ptr(), s.ld, dL.data_ptr(), cin, N, cout, cin, K, 0, cin, cout * cin, 0,
                                            part, st), 'tgmx_sgemm_tn')  # fmt: skip
        want_b = conv.bias is not None and any(n and p is conv.bias for p, n in zip(params, need[6:]))
        if want_b:
            _native.check(lib.tgmx_colsum(dout.data_ptr(), dout.stride(0), N, cout, db.data_ptr(), 0, buf(256 * cout), st), 'tgmx_colsum')
        if need[5]:
            W, _ = conv._stacked(dev)
            WT = transposed_weight(conv, W, cout, K * cin)  # [K in, out]
            if K == 1:
                _native.check(lib.tgmx_sgemm_nt(dout.data_ptr(), dout.stride(0), WT.data_ptr(), cout, dx.data_ptr(), cin, N, cin, cout, None, 0, 1, 0, 0, 0, st),
                              'tgmx_sgemm_nt')
            else:
                ldg = up4(K * cin)
                g = buf(N * ldg)
                _native.check(lib.tgmx_sgemm_nt(dout.data_ptr(), dout.stride(0), WT.data_ptr(), cout, g, ldg, N, K * cin, cout, None, 0, 1, 0, 0, 0, st),
                              'tgmx_sgemm_nt')
                _clenshaw(_graph_args(s, conv.normalization), N, cin, K, g, ldg, dx.data_ptr(), cin, buf)
        grads: List[Optional[Tensor]] = [None] * 5 + [dx if need[5] else None]
        for p, n in zip(params, need[6:]):
            grads.append(None if not n else (dL[weights[id(p)]] if id(p) in weights else db))
        return tuple(grads)


def apply_conv(conv, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], lam: float, lam_t: Optional[Tensor]) -> Tensor:
    return ChebConvFunction.apply(conv, edge_index, edge_weight, lam, lam_t, x, *param_list(conv))


def saved_graph(edge_index: Tensor, edge_weight: Optional[Tensor], lam: float, lam_t: Optional[Tensor]) -> SimpleNamespace:
    """The call's edge list as the backward's Laplacian builder reads it."""
    src, dst = _endpoints(edge_index)
    return SimpleNamespace(src=src, dst=dst, E=src.numel(), w=_edge_weight(edge_weight, src.numel()), lam=lam, lam_t=lam_t)


def _graph_args(s, normalization) -> tuple:
    """(src, dst, idx64, w, E, normalization, lambda_max, lambda_ptr) of a saved edge list, as the native entry points take them."""
    return (s.src.data_ptr(), s.dst.data_ptr(), int(s.src.dtype == torch.int64), _native.ptr(s.w), s.E, _native.CHEB_NORM[normalization], s.lam,
            _native.ptr(s.lam_t))  # fmt: skip


def _clenshaw(graph: tuple, N: int, C: int, K: int, g: int, ldg: int, out: int, ldo: int, buf) -> None:
    """L_hat^T from the edge list (skipped edges are not counted again), then the reverse recurrence in place in ``g`` (device pointers)."""
    lib, st = _native.load(), _native.stream_ptr()
    src, dst, idx64, w, E, norm, lam, lam_ptr = graph
    nbytes = lib.tgmx_cheb_workspace_bytes(E, N)
    if nbytes == 0:
        raise ValueError(f'{E} edges over {N} nodes are out of range')
    csr = (buf(N + 1, torch.int32), buf(E, torch.int32), buf(E), buf(N))
    _native.check(lib.tgmx_cheb_laplacian_t(src, dst, idx64, w, E, N, norm, lam, lam_ptr, *csr, buf(nbytes, torch.uint8), nbytes, None, st),
                  'tgmx_cheb_laplacian_t')
    nprop = lib.tgmx_cheb_propagate_scratch_floats(E, C)
    prop = buf(nprop) if nprop else None
    for k in range(K - 2, 0, -1):  # b_k = g_k + 2 L^T b_{k+1} - b_{k+2}, over g_k
        bk, two = g + 4 * k * C, k + 2 < K
        _native.check(lib.tgmx_cheb_propagate2(*csr, N, C, bk + 4 * C, ldg, bk, ldg, bk + 8 * C if two else None, ldg, 2.0, 1.0, -1.0 if two else 0.0, bk, ldg,
                                               E, prop, nprop, st), 'tgmx_cheb_propagate2')  # fmt: skip
    two = K > 2  # dH = g_0 + L^T b_1 - b_2
    _native.check(lib.tgmx_cheb_propagate2(*csr, N, C, g + 4 * C, ldg, g, ldg, g + 8 * C if two else None, ldg, 1.0, 1.0, -1.0 if two else 0.0, out, ldo, E,
                                           prop, nprop, st), 'tgmx_cheb_propagate2')  # fmt: skip


# ---- the launches of tgmx_gclstm_backward, one ctypes call each (TGMX_GCLSTM_BWD=py) --------------------------------------------------------
def backward_per_launch(t, dev) -> None:
    """What ``tgmx_gclstm_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here."""
    lib, st = _native.load(), _native.stream_ptr()
    N, C, K, cin = t.N, t.C, t.K, t.in_ch
    keep: list = []

    def buf(n: int, dtype=torch.float32) -> int:
        keep.append(torch.empty(max(1, n), dtype=dtype, device=dev))
        return keep[-1].data_ptr()

    def nt(B: int, out: int, ldo: int, cols: int) -> None:
        _native.check(lib.tgmx_sgemm_nt(dpre, 4 * C, B, t.ldwt, out, ldo, N, cols, 4 * C, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')

    dpre = buf(N * 4 * C)
    # 1. the gates
    _native.check(lib.tgmx_gclstm_gate_backward(t.pre, t.Cprev, N, C, t.dH_out, t.lddh, t.dC_out, t.lddc, dpre, t.d_Cprev, st), 'tgmx_gclstm_gate_backward')
    # 2. the parameters
    if t.d_W:  # x^T dpre_g, batched over the gates
        part = buf(lib.tgmx_sgemm_tn_workspace_bytes(N, cin, C, 4) // 4)
        _native.check(lib.tgmx_sgemm_tn(t.op, t.ldop, dpre, 4 * C, t.d_W, C, N, cin, C, 4, 0, C, cin * C, 0, part, st), 'tgmx_sgemm_tn')
    if t.d_lins:  # dpre^T Tx_k, batched over k: [K, 4, C, C]
        part = buf(lib.tgmx_sgemm_tn_workspace_bytes(N, 4 * C, C, K) // 4)
        _native.check(lib.tgmx_sgemm_tn(dpre, 4 * C, t.op + 4 * cin, t.ldop, t.d_lins, C, N, 4 * C, C, K, 0, C, 4 * C * C, 0, part, st), 'tgmx_sgemm_tn')
    if t.d_b or t.d_conv_bias:
        first = t.d_b or t.d_conv_bias
        _native.check(lib.tgmx_colsum(dpre, 4 * C, N, 4 * C, first, 0, buf(256 * 4 * C), st), 'tgmx_colsum')
        if t.d_b and t.d_conv_bias:
            _native.check(lib.tgmx_add_cols(t.d_conv_bias, 4 * C, t.d_b, 4 * C, 1, 4 * C, 0, st), 'tgmx_add_cols')  # (a copy: the same sums)
    # 3. dop = dpre Wstack, the columns somebody asked for
    if t.d_x:
        nt(t.WT, t.d_x, cin, cin)
    if t.d_H and K == 1:
        nt(t.WT + 4 * cin * t.ldwt, t.d_H, C, C)
    if t.d_H and K > 1:
        ldg = up4(K * C)
        g = buf(N * ldg)
        nt(t.WT + 4 * cin * t.ldwt, g, ldg, K * C)
        # 4. the reverse recurrence over L^T
        _clenshaw((t.src, t.dst, t.idx64, t.edge_w, t.E, t.normalization, t.lambda_max, t.lambda_ptr), N, C, K, g, ldg, t.d_H, C, buf)


__all__ = ['ChebConvFunction', 'GclstmFunction', 'apply', 'apply_conv', 'backward_per_launch', 'in_envelope', 'mode', 'saved_graph']
