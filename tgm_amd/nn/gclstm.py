"""``ChebConv`` and ``GCLSTM`` (tgm/nn/encoder/gclstm.py, https://arxiv.org/abs/1812.04206) on HIP kernels.

Same constructors, argument names and ``state_dict`` keys as the reference (``W_{i,f,c,o}``, ``b_{i,f,c,o}``, ``conv_{i,f,c,o}.lins.{k}.weight``,
``conv_{i,f,c,o}.bias``).  ``ChebConv`` is third-party to the reference (torch_geometric); it is implemented from its published definition
(``get_laplacian`` with the degree over the source index, ``2 L / lambda_max - I``, aggregation at the destination): parity unpinned upstream.

Inference (no grad): the scaled Laplacian of the snapshot is built ONCE as a CSR by destination (``tgmx_cheb_laplacian``: one stable radix
sort, no float atomics), the Chebyshev basis ``Tx_0 .. Tx_{K-1}`` is K - 1 gather SpMMs (``tgmx_cheb_propagate``) written straight into the
column slices of ONE GEMM operand, and the cell -- four convolutions sharing the basis, the four input projections, the gates -- is one
native call (``tgmx_gclstm_forward``): one GEMM against the stacked weights, one pointwise epilogue, no read back.

Training (autograd has something to track): the same forward call, with the activations the backward reads kept in buffers of the call,
and a hand-written backward as one native call (``_gclstm_train.py``, ``csrc/cheb_bwd.hip``).  Outside that path's envelope -- a gradient
asked of ``edge_weight`` or of a tensor ``lambda_max``, autocast, another dtype, ``TGMX_GCLSTM_BWD=torch`` -- the same arithmetic is
composed from torch ops on the device (``forward_composed``: ``index_add_`` and ``matmul``) and autograd does the backward.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace
from typing import List, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from . import _gclstm_train, _ops
from ._fwd_plumbing import cached_weights, carve_scratch, needs_torch, up4
from ._paramver import TransientCaches
from ._snapshot import _edge_weight, _endpoints, _Skipped, csr_scratch_sizes, propagate, propagate_scratch, scaled_laplacian

_NORMS = (None, 'sym', 'rw')
LambdaMax = Union[None, float, int, Tensor]


def _glorot(t: Tensor) -> None:
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    nn.init.uniform_(t, -bound, bound)


def _lambda(lambda_max: LambdaMax, normalization: Optional[str], device) -> Tuple[float, Optional[Tensor]]:
    """(value, device tensor): a tensor on the device is handed to the kernels as it is -- it is not read back."""
    if lambda_max is None:
        if normalization != 'sym':
            raise ValueError('ChebConv: you need to pass lambda_max in case the normalization is non-symmetric')
        return 2.0, None
    if isinstance(lambda_max, Tensor):
        if lambda_max.numel() != 1:
            raise NotImplementedError('tgm_amd ChebConv takes one lambda_max (a scalar or a one-element tensor), not one per graph of a batch')
        if lambda_max.device.type != 'cuda':
            return float(lambda_max), None
        t = lambda_max.detach().reshape(1)
        if t.device != device:
            t = t.to(device)
        return 0.0, t if t.dtype == torch.float32 else t.float()
    return float(lambda_max), None


# ---- the composed path: the same arithmetic from torch ops, with autograd ---------------------------------------------------------------------
def _composed_laplacian(edge_index: Tensor, edge_weight: Optional[Tensor], N: int, normalization: Optional[str], lam: float, lam_t: Optional[Tensor],
                        dtype, skipped: Optional[Tensor] = None):  # fmt: skip
    """(row, col, m, d) without a data-dependent shape: a dropped edge (self loop, endpoint out of range) keeps its slot with weight 0."""
    row, col = edge_index[0].long(), edge_index[1].long()
    inside = (row >= 0) & (row < N) & (col >= 0) & (col < N)
    if skipped is not None:
        skipped += (~inside).sum().to(skipped.dtype)
    keep = inside & (row != col)
    row, col = row.clamp(0, max(N - 1, 0)), col.clamp(0, max(N - 1, 0))
    w = torch.ones(row.numel(), dtype=dtype, device=row.device) if edge_weight is None else edge_weight.to(dtype).reshape(-1)
    w = torch.where(keep, w, torch.zeros_like(w))
    lmax = lam_t.to(dtype).reshape(()) if lam_t is not None else torch.tensor(lam, dtype=dtype, device=row.device)
    deg = torch.zeros(N, dtype=dtype, device=row.device).index_add_(0, row, w)
    inf = float('inf')
    if normalization == 'sym':
        dis = deg.pow(-0.5)
        dis = dis.masked_fill(dis == inf, 0)
        m, d = -(dis[row] * w * dis[col]), torch.ones_like(deg)
    elif normalization == 'rw':
        dinv = 1.0 / deg
        dinv = dinv.masked_fill(dinv == inf, 0)
        m, d = -(dinv[row] * w), torch.ones_like(deg)
    else:
        m, d = -w, deg
    m = (2.0 * m) / lmax
    m = m.masked_fill(m == inf, 0)
    d = (2.0 * d) / lmax
    d = d.masked_fill(d == inf, 0) - 1.0
    return row, col, m, d


def _composed_basis(lap, x: Tensor, K: int) -> List[Tensor]:
    row, col, m, d = lap

    def apply(t: Tensor) -> Tensor:
        return (d.unsqueeze(1) * t).index_add_(0, col, m.unsqueeze(1) * t[row])

    tx = [x]
    if K > 1:
        tx.append(apply(x))
    for _ in range(2, K):
        tx.append(2.0 * apply(tx[-1]) - tx[-2])
    return tx


class ChebConv(_Skipped, TransientCaches, nn.Module):
    """``torch_geometric.nn.ChebConv``: sum_k lins[k](Tx_k) + bias, Tx_0 = x, Tx_1 = L_hat x, Tx_k = 2 L_hat Tx_{k-1} - Tx_{k-2}."""

    def __init__(self, in_channels: int, out_channels: int, K: int, normalization: Optional[str] = 'sym', bias: bool = True) -> None:
        super().__init__()
        assert K > 0
        assert normalization in _NORMS, 'Invalid normalization'
        self.in_channels, self.out_channels, self.normalization = in_channels, out_channels, normalization
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        for lin in self.lins:
            _glorot(lin.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward_composed(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None, lambda_max: LambdaMax = None) -> Tensor:
        """The forward composed from torch ops, with autograd (device-agnostic): what the training path runs."""
        lam, lam_t = _lambda_any(lambda_max, self.normalization)
        lap = _composed_laplacian(edge_index, edge_weight, x.shape[0], self.normalization, lam, lam_t, x.dtype,
                                  self._skipped(x.device) if x.device.type == 'cuda' else None)  # fmt: skip
        tx = _composed_basis(lap, x, len(self.lins))
        out = self.lins[0](tx[0])
        for k in range(1, len(self.lins)):
            out = out + self.lins[k](tx[k])
        return out if self.bias is None else out + self.bias

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None, lambda_max: LambdaMax = None) -> Tensor:
        _native.require_device(x, 'x')
        lam, lam_t = _lambda(lambda_max, self.normalization, x.device)
        if needs_torch(self, 0.0, x):
            if x.dim() == 2 and x.shape[1] == self.in_channels and _gclstm_train.in_envelope(self, (x,), edge_weight, lambda_max):
                return _gclstm_train.apply_conv(self, x, edge_index, edge_weight, lam, lam_t)
            return self.forward_composed(x, edge_index, edge_weight, lambda_max)
        return self._forward_native(x, edge_index, edge_weight, lam, lam_t)

    def _stacked(self, dev):
        """([lins.0 | ... | lins.K-1] as [out, up4(K in)], bias), cached against the parameters' versions."""
        K, cin = len(self.lins), self.in_channels
        ld = up4(K * cin)

        def stacked():
            W = torch.zeros((self.out_channels, ld), dtype=torch.float32, device=dev)
            W[:, : K * cin] = torch.cat([lin.weight.detach().float() for lin in self.lins], dim=1)
            return W, None if self.bias is None else _ops._f32c(self.bias.detach(), 'bias')

        return cached_weights(self, stacked)

    def _forward_native(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], lam: float, lam_t: Optional[Tensor], own: bool = False):
        """``own``: the training path's call -- also returns what its backward reads (the basis ``op`` is a tensor of the call either way)."""
        x = _ops._f32c(x, 'x')
        N, K, cin, dev = x.shape[0], len(self.lins), self.in_channels, x.device
        if x.dim() != 2 or x.shape[1] != cin:
            raise ValueError(f'expected x [N, {cin}], got {list(x.shape)}')
        out = torch.empty((N, self.out_channels), dtype=torch.float32, device=dev)
        if N == 0:
            return out
        ld = up4(K * cin)
        W, b = self._stacked(dev)
        op = (torch.zeros if ld > K * cin else torch.empty)((N, ld), dtype=torch.float32, device=dev)  # [Tx_0 | ... | Tx_{K-1}]
        op[:, :cin].copy_(x)
        if K > 1:
            lap = scaled_laplacian(edge_index, edge_weight, N, self.normalization, lam, lam_t, self._skipped(dev))
            scratch = propagate_scratch(lap, cin)
            for k in range(1, K):
                sl = lambda j: op[:, j * cin : (j + 1) * cin]
                propagate(lap, sl(k - 1), sl(k), sl(k - 2) if k > 1 else None, 2.0 if k > 1 else 1.0, -1.0 if k > 1 else 0.0, scratch)
        _ops.sgemm_nt(op, W, out, bias=b, K=K * cin)
        if not own:
            return out
        s = _gclstm_train.saved_graph(edge_index, edge_weight, lam, lam_t)
        s.N, s.op, s.ld = N, op, ld
        return out, s


def _lambda_any(lambda_max: LambdaMax, normalization: Optional[str]) -> Tuple[float, Optional[Tensor]]:
    """``_lambda`` for the composed path: a tensor stays a tensor wherever it lives."""
    if isinstance(lambda_max, Tensor):
        if lambda_max.numel() != 1:
            raise NotImplementedError('tgm_amd ChebConv takes one lambda_max (a scalar or a one-element tensor), not one per graph of a batch')
        return 0.0, lambda_max.detach()
    return _lambda(lambda_max, normalization, None)


class GCLSTM(_Skipped, TransientCaches, nn.Module):
    """The GC-LSTM cell: an LSTM whose hidden-state term of every gate is a Chebyshev graph convolution of ``H``,
    ``gate = act(X W_g + ChebConv_g(H) + b_g)`` for g in i, f, c, o; ``C' = F C + I T``, ``H' = O tanh(C')``.

    ``in_channels`` / ``out_channels``: widths of ``node_x`` and of the states; ``K``: the number of Chebyshev terms; ``normalization``:
    ``'sym'`` (default), ``'rw'`` or ``None``, the last two need ``lambda_max`` in :meth:`forward`; ``bias=False`` leaves the convolutions
    without their additive bias (``b_g`` stays).
    """

    def __init__(self, in_channels: int, out_channels: int, K: int, normalization: Optional[str] = 'sym', bias: bool = True) -> None:
        super().__init__()
        self.in_channels, self.out_channels, self.K, self.normalization, self.bias = in_channels, out_channels, K, normalization, bias
        for g in 'ifco':  # (the reference's order of registration: conv, W, b per gate)
            setattr(self, f'conv_{g}', ChebConv(out_channels, out_channels, K=K, normalization=normalization, bias=bias))
            setattr(self, f'W_{g}', nn.Parameter(torch.empty(in_channels, out_channels)))
            setattr(self, f'b_{g}', nn.Parameter(torch.empty(1, out_channels)))
        for g in 'ifco':
            _glorot(getattr(self, f'W_{g}'))
            nn.init.zeros_(getattr(self, f'b_{g}'))

    def _gates(self):
        return [(getattr(self, f'W_{g}'), getattr(self, f'b_{g}'), getattr(self, f'conv_{g}')) for g in 'ifco']

    def forward_composed(self, node_x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None, H: Optional[Tensor] = None,
                         C: Optional[Tensor] = None, lambda_max: LambdaMax = None) -> Tuple[Tensor, Tensor]:  # fmt: skip
        """The cell composed from torch ops, with autograd (device-agnostic): what the training path runs.  The four convolutions share one
        Laplacian and one Chebyshev basis of H."""
        N, Co = node_x.shape[0], self.out_channels
        H = torch.zeros(N, Co, dtype=node_x.dtype, device=node_x.device) if H is None else H
        C = torch.zeros(N, Co, dtype=node_x.dtype, device=node_x.device) if C is None else C
        lam, lam_t = _lambda_any(lambda_max, self.normalization)
        lap = _composed_laplacian(edge_index, edge_weight, N, self.normalization, lam, lam_t, node_x.dtype,
                                  self._skipped(node_x.device) if node_x.device.type == 'cuda' else None)  # fmt: skip
        tx = _composed_basis(lap, H, self.K)
        pre = []
        for W, b, conv in self._gates():
            g = conv.lins[0](tx[0])
            for k in range(1, self.K):
                g = g + conv.lins[k](tx[k])
            if conv.bias is not None:
                g = g + conv.bias
            pre.append(torch.matmul(node_x, W) + g + b)
        I, F, T, O = torch.sigmoid(pre[0]), torch.sigmoid(pre[1]), torch.tanh(pre[2]), torch.sigmoid(pre[3])
        C = F * C + I * T
        return O * torch.tanh(C), C

    def forward(self, node_x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None, H: Optional[Tensor] = None,
                C: Optional[Tensor] = None, lambda_max: LambdaMax = None) -> Tuple[Tensor, Tensor]:  # fmt: skip
        """Returns the hidden state and the cell state of every node, ``(H, C)``; ``H`` / ``C`` of ``None`` are zeros."""
        _native.require_device(node_x, 'node_x')
        lam, lam_t = _lambda(lambda_max, self.normalization, node_x.device)
        if node_x.dim() != 2 or node_x.shape[1] != self.in_channels:
            raise ValueError(f'expected node_x [N, {self.in_channels}], got {list(node_x.shape)}')
        states = [t for t in (H, C) if t is not None]
        if needs_torch(self, 0.0, node_x, *states):
            if _gclstm_train.in_envelope(self, (node_x, *states), edge_weight, lambda_max):
                return _gclstm_train.apply(self, node_x, edge_index, edge_weight, H, C, lam, lam_t)
            return self.forward_composed(node_x, edge_index, edge_weight, H, C, lambda_max)
        return self._forward_native(node_x, edge_index, edge_weight, H, C, lam, lam_t)

    def _stacked(self, dev):
        """(W [4C, up4(in + K C)], b [4C]), cached against the parameters' versions.  Rows of gate g: [W_g^T | lins_g,0 | ... | lins_g,K-1],
        bias b_g + conv_g.bias."""
        Co, K, cin = self.out_channels, self.K, self.in_channels
        width = cin + K * Co
        f32 = dict(dtype=torch.float32, device=dev)

        def stacked():
            W = torch.zeros((4 * Co, up4(width)), **f32)
            b = torch.empty(4 * Co, **f32)
            for g, (Wg, bg, conv) in enumerate(self._gates()):
                rows = slice(g * Co, (g + 1) * Co)
                W[rows, :cin] = Wg.detach().t()
                W[rows, cin:width] = torch.cat([lin.weight.detach().float() for lin in conv.lins], dim=1)
                b[rows] = bg.detach().reshape(-1) if conv.bias is None else bg.detach().reshape(-1) + conv.bias.detach()
            return W, b

        return cached_weights(self, stacked)

    def _forward_native(self, node_x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], H: Optional[Tensor], C: Optional[Tensor], lam: float,
                        lam_t: Optional[Tensor], own: bool = False):  # fmt: skip
        """``own``: the training path's call -- ``op`` and ``pre`` are tensors of this call instead of regions of the module's scratch, and
        what the backward reads is returned as a third value."""
        lib = _native.load()
        x = _ops._f32c(node_x, 'node_x')
        N, Co, K, cin, dev = x.shape[0], self.out_channels, self.K, self.in_channels, x.device
        f32 = dict(dtype=torch.float32, device=dev)
        H_out, C_out = torch.empty((N, Co), **f32), torch.empty((N, Co), **f32)
        if N == 0:
            return H_out, C_out
        H = torch.zeros((N, Co), **f32) if H is None else _ops._f32c(H, 'H')
        C = torch.zeros((N, Co), **f32) if C is None else _ops._f32c(C, 'C')
        if tuple(H.shape) != (N, Co) or tuple(C.shape) != (N, Co):
            raise ValueError(f'expected H and C [{N}, {Co}], got {list(H.shape)} and {list(C.shape)}')
        width = cin + K * Co
        ld = up4(width)

        W, b = self._stacked(dev)
        src, dst = _endpoints(edge_index)
        E = src.numel()
        w = _edge_weight(edge_weight, E)
        csr, nprop = [N + 1, 0, 0, N, 0], 0  # K = 1: no Laplacian is built
        if K > 1:
            nprop = lib.tgmx_cheb_propagate_scratch_floats(E, Co)
            csr = csr_scratch_sizes(E, N, lib.tgmx_cheb_workspace_bytes(E, N), 'GCLSTM')
        # indptr, cols, vals, diag, sort workspace, op, pre, the propagate's chunk sums
        bufs = carve_scratch(self, csr + ([0, 0] if own else [N * ld, N * 4 * Co]) + [nprop], dev)
        if own:
            bufs[5], bufs[6] = torch.empty(N * ld, **f32), torch.empty(N * 4 * Co, **f32)
        d = self.__dict__
        a = d.get('_tgmx_args')
        if a is None:
            a = d['_tgmx_args'] = _native.GclstmFwd()
        a.x, a.N, a.in_ch, a.C, a.K, a.normalization = x.data_ptr(), N, cin, Co, K, _native.CHEB_NORM[self.normalization]
        a.src, a.dst, a.edge_w, a.E, a.idx64 = src.data_ptr(), dst.data_ptr(), _native.ptr(w), E, 1 if src.dtype == torch.int64 else 0
        a.lambda_max, a.lambda_ptr = lam, _native.ptr(lam_t)
        a.W, a.b, a.ldw = W.data_ptr(), b.data_ptr(), ld
        a.H, a.Cprev = H.data_ptr(), C.data_ptr()
        a.indptr, a.cols, a.vals, a.diag, a.lap_ws = (t.data_ptr() for t in bufs[:5])
        a.lap_ws_bytes, a.skipped = bufs[4].numel() * 4, self._skipped(dev).data_ptr()
        a.op, a.ldop, a.pre = bufs[5].data_ptr(), ld, bufs[6].data_ptr()
        a.prop_ws, a.prop_ws_floats = (bufs[7].data_ptr() if nprop else None), nprop
        a.H_out, a.C_out = H_out.data_ptr(), C_out.data_ptr()
        _native.check(lib.tgmx_gclstm_forward(ctypes.byref(a), _native.stream_ptr()), 'tgmx_gclstm_forward')
        if not own:
            return H_out, C_out
        s = SimpleNamespace(N=N, op=bufs[5], pre=bufs[6], ld=ld, C=C, src=src, dst=dst, E=E, w=w, lam=lam, lam_t=lam_t)
        return H_out, C_out, s
