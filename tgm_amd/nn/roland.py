"""``ROLAND`` (tgm/nn/encoder/roland.py, https://arxiv.org/abs/2208.07239) on HIP kernels.

Same constructor, argument names and ``state_dict`` keys as the reference (``conv{1,2}.lin.weight``, ``conv{1,2}.bias``, ``tau`` for
``'learnable'``, ``gru{1,2}.{weight,bias}_{ih,hh}``, ``mlp{1,2}.{weight,bias}``).  ``GCNConv`` is third-party to the reference
(torch_geometric); it is implemented from its published definition: parity unpinned upstream.

Every branch of the reference's forward ends in ``torch.Tensor(... .detach())``: its outputs never carry a gradient, in train mode as
well.  The native forward is therefore the whole model, not an inference path beside a training path: GCN's normalised adjacency of the
snapshot is built ONCE as a CSR by destination (``tgmx_gcn_norm_csr``: one stable radix sort, no float atomics), each layer is one GEMM
and one gather SpMM whose epilogue adds the bias, applies the relu and -- for ``'moving'``, ``'learnable'`` and ``None`` -- blends in
the previous embedding (``tgmx_gcn_propagate``), and the whole snapshot is one native call (``tgmx_roland_forward``), no read back.
Only active dropout needs torch ops: ``training and dropout > 0`` takes :meth:`ROLAND.forward_composed` (device-agnostic, also detached).

Kept from the reference: embeddings passed to ``forward`` are COPIED into the module and a later call without them reuses the copy; the
forward does not store its own outputs; ``'moving'`` starts at ``tau = 0`` and takes ``float32(prev / (prev + cur))`` only when both
edge counts are given.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .. import _native
from . import _ops
from ._fwd_plumbing import cached_block, carve_scratch
from ._paramver import TransientCaches
from ._snapshot import _endpoints, _Skipped, csr_scratch_sizes
from .tgcn import GCNConv, composed_gcn_conv

_UPDATES = ('moving', 'learnable', 'gru', 'mlp', None)


class ROLAND(_Skipped, TransientCaches, nn.Module):
    """Two GCN layers whose outputs are merged with the node embeddings of the previous snapshot, layer by layer.

    ``input_channel`` / ``out_channel``: widths of ``node_x`` and of the embeddings; ``num_nodes``: rows of the embedding state;
    ``dropout``: rate after each layer's relu (training only); ``update``: ``'moving'`` (tau from the edge counts), ``'learnable'`` (tau a
    parameter), ``'gru'``, ``'mlp'`` or ``None`` (the constructor's ``tau``).
    """

    def __init__(self, input_channel: int, out_channel: int, num_nodes: int, dropout: float = 0.0, update: Optional[str] = 'learnable',
                 tau: float = 0.5) -> None:  # fmt: skip
        assert update in _UPDATES
        super().__init__()
        self.conv1 = GCNConv(input_channel, out_channel)
        self.conv2 = GCNConv(out_channel, out_channel)
        self.dropout = dropout
        self.update = update
        if update == 'moving':
            self.tau = torch.zeros(1)
        elif update == 'learnable':
            self.tau = nn.Parameter(torch.zeros(1))
        elif update == 'gru':
            self.gru1 = nn.GRUCell(out_channel, out_channel)
            self.gru2 = nn.GRUCell(out_channel, out_channel)
        elif update == 'mlp':
            self.mlp1 = nn.Linear(out_channel * 2, out_channel)
            self.mlp2 = nn.Linear(out_channel * 2, out_channel)
        else:
            assert tau >= 0 and tau <= 1
            self.tau = torch.tensor([tau], dtype=torch.float32)
        self.input_channel, self.out_channel, self.num_nodes = input_channel, out_channel, num_nodes
        self.previous_embeddings = [torch.zeros(num_nodes, out_channel), torch.zeros(num_nodes, out_channel)]

    def reset_parameters(self) -> None:
        self.conv1.reset_parameters()
        self.conv2.reset_parameters()

    # ---- the state both paths share ---------------------------------------------------------------------------------------------------------
    def _moving_tau(self, num_current_edges, num_previous_edges) -> None:
        if self.update == 'moving' and num_current_edges is not None and num_previous_edges is not None:
            self.tau = torch.tensor([num_previous_edges / (num_previous_edges + num_current_edges)], dtype=torch.float32)  # the past's weight

    def _check_inputs(self, node_x: Tensor, previous_embeddings: Optional[Sequence[Tensor]]) -> None:
        if node_x.dim() != 2 or node_x.shape[1] != self.input_channel:
            raise ValueError(f'expected node_x [N, {self.input_channel}], got {list(node_x.shape)}')
        if previous_embeddings is not None:
            if len(previous_embeddings) != 2:
                raise ValueError('expected the two previous embeddings, one per layer')
            for t in previous_embeddings:
                if t.dim() != 2 or t.shape[1] != self.out_channel:
                    raise ValueError(f'expected previous embeddings [N, {self.out_channel}], got {list(t.shape)}')
        rows = self.previous_embeddings[0].shape[0] if previous_embeddings is None else previous_embeddings[0].shape[0]
        if rows != node_x.shape[0] or (previous_embeddings is not None and previous_embeddings[1].shape[0] != rows):
            raise ValueError(f'node_x has {node_x.shape[0]} rows, the embedding state {rows}')

    # ---- the composed path: the same arithmetic from torch ops ------------------------------------------------------------------------------
    def forward_composed(self, node_x: Tensor, edge_index: Tensor, previous_embeddings: Optional[List[Tensor]] = None,
                         num_current_edges: Optional[int] = None, num_previous_edges: Optional[int] = None) -> List[Tensor]:  # fmt: skip
        """The forward composed from torch ops (device-agnostic): what runs when dropout is active.  Detached, as the reference's."""
        self._check_inputs(node_x, previous_embeddings)
        if previous_embeddings is not None:
            self.previous_embeddings = [previous_embeddings[0].detach().clone(), previous_embeddings[1].detach().clone()]
        self._moving_tau(num_current_edges, num_previous_edges)
        skipped = self._skipped(node_x.device) if node_x.device.type == 'cuda' else None
        out: List[Tensor] = []
        h = node_x
        for l, conv in enumerate((self.conv1, self.conv2)):
            h = F.relu(composed_gcn_conv(conv, h, edge_index, skipped))
            h = F.dropout(h, p=self.dropout, training=self.training)
            prev = self.previous_embeddings[l].to(device=h.device, dtype=h.dtype)
            if self.update == 'gru':
                h = getattr(self, f'gru{l + 1}')(h, prev)
            elif self.update == 'mlp':
                h = getattr(self, f'mlp{l + 1}')(torch.cat((h, prev), dim=1))
            else:
                tau = self.tau.to(device=h.device, dtype=h.dtype)
                h = tau * prev + (1 - tau) * h
            h = h.detach()
            out.append(h)
            skipped = None  # (the second layer reads the same edges)
        return [out[0].clone(), out[1].clone()]

    # ---- the native path ----------------------------------------------------------------------------------------------------------------------
    def forward(self, node_x: Tensor, edge_index: Tensor, previous_embeddings: Optional[List[Tensor]] = None,
                num_current_edges: Optional[int] = None, num_previous_edges: Optional[int] = None) -> List[Tensor]:  # fmt: skip
        """Returns the embeddings after the first and the second layer, ``[H0, H1]`` (the last is the model's embedding).  Neither requires
        grad.  ``previous_embeddings``: the two states to merge with, copied into the module; ``None`` reuses the last ones passed (zeros
        before any).  ``num_current_edges`` / ``num_previous_edges``: ``'moving'`` takes its tau from them when both are given."""
        _native.require_device(node_x, 'node_x')
        if self.training and self.dropout > 0:
            return self.forward_composed(node_x, edge_index, previous_embeddings, num_current_edges, num_previous_edges)
        self._check_inputs(node_x, previous_embeddings)
        self._moving_tau(num_current_edges, num_previous_edges)
        lib = _native.load()
        x = _ops._f32c(node_x.detach(), 'node_x')
        N, C, cin, dev = x.shape[0], self.out_channel, self.input_channel, x.device
        f32 = dict(dtype=torch.float32, device=dev)
        out = [torch.empty((N, C), **f32), torch.empty((N, C), **f32)]
        if N == 0:
            if previous_embeddings is not None:
                self.previous_embeddings = [previous_embeddings[0].detach().clone(), previous_embeddings[1].detach().clone()]
            return out
        src, dst = _endpoints(edge_index)
        E = src.numel()
        csr = csr_scratch_sizes(E, N, lib.tgmx_gcn_workspace_bytes(E, N), 'ROLAND')
        nprop = lib.tgmx_cheb_propagate_scratch_floats(E, C)
        mode = _native.ROLAND_UPDATE[self.update]
        a, _keep = cached_block(self, self._weights)
        a.x, a.N, a.in_ch, a.C, a.update, a.add_self_loops, a.fill = x.data_ptr(), N, cin, C, mode, 1, 1.0
        a.src, a.dst, a.E, a.idx64 = src.data_ptr(), dst.data_ptr(), E, 1 if src.dtype == torch.int64 else 0
        gru = 3 * N * C if self.update == 'gru' else 0
        # indptr, cols, vals, diag, sort workspace, the propagate's chunk sums, xw, gi, gh
        bufs = carve_scratch(self, csr + [nprop, N * C, gru, gru], dev)
        a.indptr, a.cols, a.vals, a.diag, a.norm_ws = (t.data_ptr() for t in bufs[:5])
        a.norm_ws_bytes, a.skipped = bufs[4].numel() * 4, self._skipped(dev).data_ptr()
        a.prop_ws, a.prop_ws_floats = (bufs[5].data_ptr() if nprop else None), nprop
        a.xw, a.gi, a.gh = bufs[6].data_ptr(), (bufs[7].data_ptr() if gru else None), (bufs[8].data_ptr() if gru else None)
        hold = []  # tensors the call reads that nothing else keeps alive
        if mode == 0:
            self._state_tau(a, previous_embeddings, N, C, f32, hold)
        else:
            self._state_operands(a, previous_embeddings, N, C, f32)
        a.out[0], a.out[1] = out[0].data_ptr(), out[1].data_ptr()
        _native.check(lib.tgmx_roland_forward(ctypes.byref(a), _native.stream_ptr()), 'tgmx_roland_forward')
        return out

    def _weights(self, f32):
        """The argument block with every weight pointer filled in (cached against the parameters' versions)."""
        a = _native.RolandFwd()
        for l, conv in enumerate((self.conv1, self.conv2)):
            a.conv_w[l], a.ldw[l], a.conv_b[l] = f32(conv.lin.weight), conv.lin.weight.shape[1], f32(conv.bias, 'bias')
            if self.update == 'mlp':
                lin = getattr(self, f'mlp{l + 1}')
                a.mlp_w[l], a.mlp_b[l] = f32(lin.weight), f32(lin.bias, 'bias')
            elif self.update == 'gru':
                cell = getattr(self, f'gru{l + 1}')
                a.w_ih[l], a.w_hh[l], a.b_ih[l], a.b_hh[l] = f32(cell.weight_ih), f32(cell.weight_hh), f32(cell.bias_ih, 'bias'), f32(cell.bias_hh, 'bias')
        return a

    def _state_tau(self, a, previous_embeddings, N: int, C: int, f32, hold: list) -> None:
        """'moving' / 'learnable' / None: the update is the propagate's epilogue.  Embeddings passed in are read where they are and copied
        into the module's state by the same epilogue."""
        state = self.previous_embeddings
        if previous_embeddings is None:
            for l in range(2):
                s = state[l]
                if s.device != f32['device'] or s.dtype != torch.float32 or not s.is_contiguous():
                    s = state[l] = s.to(**f32).contiguous()
                a.prev[l], a.prev_copy[l] = s.data_ptr(), None
        else:
            for l in range(2):
                p = _ops._f32c(previous_embeddings[l].detach(), 'previous_embeddings')
                s = state[l]
                if tuple(s.shape) != (N, C) or s.device != p.device or s.dtype != torch.float32 or not s.is_contiguous():
                    s = state[l] = torch.empty((N, C), **f32)
                hold.append(p)
                a.prev[l], a.prev_copy[l] = p.data_ptr(), (None if p.data_ptr() == s.data_ptr() else s.data_ptr())
        a.ldp = C
        if self.update == 'learnable':
            t = self.tau.detach()
            t = t if t.dtype == torch.float32 else t.float()
            _native.require_device(t, 'tau')
            hold.append(t)
            a.tau, a.tau_ptr = 0.0, t.data_ptr()  # a Parameter on the device: never read back
        else:
            a.tau, a.tau_ptr = float(self.tau), None  # (a host tensor)

    def _state_operands(self, a, previous_embeddings, N: int, C: int, f32) -> None:
        """'mlp' / 'gru': layer l's update reads [relu(conv_l) | prev_l] as one [N, 2C] operand.  The module keeps its state IN the right
        column slice of two such operands, so copying embeddings into the module and filling the operand are the same copy."""
        ops = self.__dict__.get('_tgmx_ops')
        state = self.previous_embeddings
        for l in range(2):
            op = None if ops is None else ops[l]
            s = state[l] if previous_embeddings is None else previous_embeddings[l].detach()
            ours = op is not None and tuple(op.shape) == (N, 2 * C) and op.device == f32['device']
            if not (ours and previous_embeddings is None and state[l].data_ptr() == op.data_ptr() + 4 * C and state[l].stride(0) == 2 * C):
                if not ours:
                    op = torch.empty((N, 2 * C), **f32)
                    if ops is None:
                        ops = self.__dict__['_tgmx_ops'] = [None, None]
                    ops[l] = op
                op[:, C:].copy_(s)
                state[l] = op[:, C:]
            a.op[l] = op.data_ptr()

    def extra_repr(self) -> str:
        return f'update={self.update!r}, dropout={self.dropout}, num_nodes={self.num_nodes}'
