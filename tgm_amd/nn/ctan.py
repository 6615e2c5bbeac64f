"""CTAN (tgm/nn/encoder/ctan.py, https://arxiv.org/abs/2406.02740) on HIP kernels: ``CTAN`` and ``CTANMemory``.

Same constructors, argument names, buffers and ``state_dict`` keys as the reference (``time_enc.lin.*``, ``enc_x.*``, ``aconv.W``,
``aconv.bias``, ``aconv.eye``, ``aconv.phi.lin_{key,query,value}.*``, ``aconv.phi.lin_edge.weight``), so ``load_state_dict(strict=True)``
works both ways.  The PyG parts -- ``AntiSymmetricConv``, ``TransformerConv(heads=1, root_weight=False)``, ``TimeEncoder`` -- are
built from their published definitions (2.6.1); PyG is third-party to the reference and parity against it is unpinned.

Inference (no grad): the whole forward is ONE native call (``tgmx_ctan_forward``, csrc/ctan.hip).  What does not change over
``AntiSymmetricConv``'s iterations -- the edge encoding, the ``[E, D+T] x [D+T, M]`` edge projection, the grouping of the edges by target
-- runs once; an iteration is one batched GEMM over the stacked weights ``[W_query, W_key, W_value, A]`` (``A = W - W^T - gamma I`` in the
slot TransformerConv's skip projection has in ``tgmx_tconv_forward``) and one attention launch whose epilogue is
``x <- x + epsilon tanh(phi + x A^T + bias)``.

Training (``_ctan_train.py``): under gradients the forward is the same call in its saving form -- the bits of the no-grad output -- and
``loss.backward()`` is ONE native call (``tgmx_ctan_backward``, csrc/ctan_bwd.hip): a target pass and a source pass per iteration, no float
atomics.  Outside its envelope (``_ctan_train.in_envelope``; ``TGMX_CTAN_BWD=torch``) the call goes to :meth:`CTAN.forward_composed`.

``CTANMemory.update_state`` is two launches over the 2B positions of ``cat[src, pos_dst]`` (``tgmx_ctan_memory_update``): no
``unique``, no dense score matrix, no read back; out-of-range ids are skipped and reported by :meth:`CTANMemory.check`.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from . import _ctan_train, _ops
from ._paramver import TransientCaches, param_key, param_list
from .tgn import LastAggregator, MeanAggregator

_INT64_MIN = -(1 << 63)


class TimeEncoder(nn.Module):
    """``torch_geometric.nn.models.tgn.TimeEncoder``: cos(Linear(1, out_channels)(t))."""

    def __init__(self, out_channels: int) -> None:
        super().__init__()
        self.out_channels = out_channels
        self.lin = nn.Linear(1, out_channels)

    def reset_parameters(self) -> None:
        self.lin.reset_parameters()

    def forward(self, t: Tensor) -> Tensor:
        return self.lin(t.view(-1, 1)).cos()


class _Phi(nn.Module):
    """The parameters of ``TransformerConv(memory_dim, memory_dim, heads=1, edge_dim=edge_dim + time_dim, root_weight=False)``."""

    def __init__(self, channels: int, edge_dim: int) -> None:
        super().__init__()
        self.in_channels = self.out_channels = channels
        self.heads, self.edge_dim = 1, edge_dim
        self.lin_key = nn.Linear(channels, channels)
        self.lin_query = nn.Linear(channels, channels)
        self.lin_value = nn.Linear(channels, channels)
        self.lin_edge = nn.Linear(edge_dim, channels, bias=False)

    def reset_parameters(self) -> None:
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge):
            lin.reset_parameters()


class AntiSymmetricConv(nn.Module):
    """The parameters of ``torch_geometric.nn.AntiSymmetricConv(in_channels, phi, num_iters, epsilon, gamma)`` (act = tanh, bias)."""

    def __init__(self, in_channels: int, phi: nn.Module, num_iters: int = 1, epsilon: float = 0.1, gamma: float = 0.1) -> None:
        super().__init__()
        self.in_channels, self.num_iters, self.epsilon, self.gamma = in_channels, num_iters, epsilon, gamma
        self.phi = phi
        self.W = nn.Parameter(torch.empty(in_channels, in_channels))
        self.register_buffer('eye', torch.eye(in_channels))
        self.bias = nn.Parameter(torch.empty(in_channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.W, a=math.sqrt(5))
        self.phi.reset_parameters()
        nn.init.zeros_(self.bias)


def _grow(buf, numel: int, dtype, dev) -> Tensor:
    if buf is None or buf.device != dev or buf.numel() < numel:
        buf = torch.empty(max(numel, 1), dtype=dtype, device=dev)
    return buf


class CTAN(TransientCaches, nn.Module):
    """An implementation of CTAN.

    Args:
        edge_dim (int): Dimension of edge features.
        memory_dim (int): Dimension of memory embeddings.
        time_dim (int): Dimension of time encodings.
        node_dim (int): Dimension of static/dynamic node features.
        num_iters (int): Number of AntiSymmetricConv layers.
        mean_delta_t (float): Mean delta time between edge events (used to normalize time signal).
        std_delta_t (float): Std delta time between edge events (used to normalize time signal).
        epsilon (float): Discretization step size for AntiSymmetricConv.
        gamma (float): The strength of the diffusion in the AntiSymmetricConv.
    """

    _TRANSIENT = ('_fwd_args', '_stacked', '_ws')

    def __init__(self, edge_dim: int, memory_dim: int, time_dim: int, node_dim: int, num_iters: int = 1, mean_delta_t: float = 0.0,
                 std_delta_t: float = 1.0, epsilon: float = 0.1, gamma: float = 0.1) -> None:  # fmt: skip
        super().__init__()
        self.mean_delta_t = mean_delta_t
        self.std_delta_t = std_delta_t
        self.time_enc = TimeEncoder(time_dim)
        self.enc_x = nn.Linear(memory_dim + node_dim, memory_dim)
        phi = _Phi(memory_dim, edge_dim + time_dim)
        self.aconv = AntiSymmetricConv(memory_dim, phi, num_iters=num_iters, epsilon=epsilon, gamma=gamma)

    # ---- the same arithmetic from torch ops on the device ----------------------------------------------------------------------------
    def forward_composed(self, node_x: Tensor, last_update: Tensor, edge_index: Tensor, t: Tensor, msg: Tensor) -> Tensor:
        """The forward composed from torch ops, with autograd: what training runs outside the native envelope and what the native paths are
        timed and tested against."""
        aconv, phi = self.aconv, self.aconv.phi
        src, tgt = edge_index[0].long(), edge_index[1].long()
        rel_t = (last_update[src] - t).abs()
        rel_t = ((rel_t - self.mean_delta_t) / self.std_delta_t).to(node_x.dtype)
        x = self.enc_x(node_x)
        edge_attr = torch.cat([msg, self.time_enc(rel_t)], dim=-1)
        U, M = x.shape
        A = aconv.W - aconv.W.t() - aconv.gamma * aconv.eye
        e = phi.lin_edge(edge_attr)  # the same for every iteration
        for _ in range(aconv.num_iters):
            q, k, v = phi.lin_query(x), phi.lin_key(x), phi.lin_value(x)
            h = x @ A.t()
            if e.shape[0]:
                score = (q[tgt] * (k[src] + e)).sum(-1) / math.sqrt(M)
                top = torch.full((U,), float('-inf'), dtype=score.dtype, device=score.device).scatter_reduce(0, tgt, score.detach(), 'amax')
                w = (score - top[tgt]).exp()
                den = torch.zeros(U, dtype=w.dtype, device=w.device).index_add_(0, tgt, w)
                alpha = w / den[tgt]
                h = h + torch.zeros_like(x).index_add_(0, tgt, alpha.unsqueeze(-1) * (v[src] + e))
            x = x + aconv.epsilon * torch.tanh(h + aconv.bias)
        return torch.tanh(x)

    # ---- one native call ------------------------------------------------------------------------------------------------------------
    def _stacked_projections(self) -> Tuple[Tensor, Tensor]:
        """[4, M, M] = [W_query, W_key, W_value, A] and [4, M] = [b_query, b_key, b_value, bias], rebuilt only when a parameter was reallocated or
        modified in place (optimizer step, load_state_dict)."""
        aconv, phi = self.aconv, self.aconv.phi
        lins = (phi.lin_query, phi.lin_key, phi.lin_value)
        key = (param_key([p for lin in lins for p in (lin.weight, lin.bias)] + [aconv.W, aconv.bias]), float(aconv.gamma))
        cached = getattr(self, '_stacked', None)
        if cached is None or cached[0] != key:
            W = aconv.W.detach().float()
            A = W - W.t() - aconv.gamma * aconv.eye.float()
            W4 = torch.stack([lin.weight.detach().float() for lin in lins] + [A]).contiguous()
            b4 = torch.stack([lin.bias.detach().float() for lin in lins] + [aconv.bias.detach().float()]).contiguous()
            cached = self._stacked = (key, W4, b4)
        return cached[1], cached[2]

    def forward(self, node_x: Tensor, last_update: Tensor, edge_index: Tensor, t: Tensor, msg: Tensor) -> Tensor:
        """Forward pass.

        Args:
            node_x (PyTorch Float Tensor): Node features, ``[U, memory_dim + node_dim]``.
            last_update (PyTorch Tensor): Last memory update timestamps, ``[U]``.
            edge_index (PyTorch Tensor): Graph edge indices ``[2, E]`` (int32 or int64), messages flow from row 0 to row 1.
            t (PyTorch Tensor): Graph edge timestamps.
            msg (PyTorch Tensor): Edge features (any real dtype).

        Returns:
            (PyTorch Float Tensor): Embeddings for the batch of node ids.
        """
        _native.require_device(node_x, 'CTAN: node_x')
        _native.load()
        if torch.is_grad_enabled() and (node_x.requires_grad or any(p.requires_grad for p in param_list(self))):
            if _ctan_train.in_envelope(self, node_x, msg):
                return _ctan_train.apply(self, node_x, last_update, edge_index, t, msg)
            return self.forward_composed(node_x, last_update, edge_index, t, msg)
        return self._forward_native(node_x, last_update, edge_index, t, msg)[0]

    def _forward_native(self, node_x: Tensor, last_update: Tensor, edge_index: Tensor, t: Tensor, msg: Tensor, own: bool = False):
        """``(out, saved)``.  ``own``: the saving forward -- every iteration's x and what is produced once per call (edge_attr, eproj, the
        clamped sources, the grouping by target) go to tensors that belong to THIS call and come back in ``saved``; the projections' buffer
        and the sort workspace are dead after the forward and stay in the module's shared scratch."""
        lib = _native.load()
        aconv, phi = self.aconv, self.aconv.phi
        x_in = _ops._f32c(node_x, 'node_x')
        dev, U, M = x_in.device, x_in.shape[0], aconv.in_channels
        E, T = edge_index.shape[1], self.time_enc.out_channels
        msg = _ops._f32c(msg, 'msg')
        D = msg.shape[1]
        if x_in.shape[1] != self.enc_x.in_features or D + T != phi.edge_dim:
            raise ValueError(f'CTAN: node_x has {x_in.shape[1]} columns and msg {D}; expected {self.enc_x.in_features} and {phi.edge_dim - T}')
        out = torch.empty((U, M), dtype=torch.float32, device=dev)
        if U == 0:
            return out, None
        ei = edge_index.to(torch.int64)
        src, tgt = ei[0].contiguous(), ei[1].contiguous()
        lu64, t64 = last_update.to(torch.int64).contiguous(), t.to(torch.int64).contiguous()
        W4, b4 = self._stacked_projections()
        need = int(lib.tgmx_segment_sort_workspace_bytes(E))
        ws = getattr(self, '_ws', None) or {}
        ws['sort'] = _grow(ws.get('sort'), need, torch.uint8, dev)
        if ws.get('status') is None or ws['status'].device != dev:
            ws['status'] = torch.zeros(1, dtype=torch.int32, device=dev)
        r4 = lambda n: (n + 3) & ~3  # every block at a 16-byte boundary: the attention's vector loads ask for it
        o_ep = r4(E * (D + T))
        o_x = o_ep + r4(E * M)
        o_qk = o_x + r4(U * M)
        fl = ws['fl'] = _grow(ws.get('fl'), o_qk + 4 * U * M, torch.float32, dev)  # edge_attr | eproj | x | qkvs
        ints = ws['ints'] = _grow(ws.get('ints'), 2 * E + 2 * U, torch.int64, dev)  # src_ok | order | seg_lo | seg_hi
        self._ws = ws
        saved = None
        if own:
            n_it = int(aconv.num_iters)
            kept = torch.empty(max(o_x, 1), dtype=torch.float32, device=dev)  # edge_attr | eproj
            kept_i = torch.empty(max(2 * E + 2 * U, 1), dtype=torch.int64, device=dev)
            x_save = torch.empty((max(n_it, 1), U, M), dtype=torch.float32, device=dev)
            saved = SimpleNamespace(U=U, E=E, M=M, D=D, T=T, in_ch=x_in.shape[1], num_iters=n_it, node_x=x_in, last_update=lu64, t=t64, W4=W4, b4=b4,
                                    kept=kept, kept_i=kept_i, x_save=x_save, o_ep=o_ep)
        a = getattr(self, '_fwd_args', None)
        if a is None:
            a = self._fwd_args = _native.CtanFwd()
        f0, i0 = fl.data_ptr(), ints.data_ptr()
        a.node_x, a.U, a.in_ch, a.M, a.last_update = x_in.data_ptr(), U, x_in.shape[1], M, lu64.data_ptr()
        a.src, a.tgt, a.t, a.msg, a.E, a.D, a.T = src.data_ptr(), tgt.data_ptr(), t64.data_ptr(), msg.data_ptr(), E, D, T
        a.tw, a.tb = self.time_enc.lin.weight.detach().data_ptr(), self.time_enc.lin.bias.detach().data_ptr()
        a.W_x, a.b_x = self.enc_x.weight.detach().data_ptr(), self.enc_x.bias.detach().data_ptr()
        a.W4, a.b4, a.W_edge = W4.data_ptr(), b4.data_ptr(), phi.lin_edge.weight.detach().data_ptr()
        a.num_iters, a.epsilon, a.mean_delta_t, a.std_delta_t = int(aconv.num_iters), float(aconv.epsilon), float(self.mean_delta_t), float(self.std_delta_t)
        a.x, a.qkvs, a.x_save = f0 + 4 * o_x, f0 + 4 * o_qk, None
        if own:
            f0, i0, a.x_save = kept.data_ptr(), kept_i.data_ptr(), x_save.data_ptr()
        a.edge_attr, a.eproj = f0, f0 + 4 * o_ep
        a.src_ok, a.order, a.seg_lo, a.seg_hi = i0, i0 + 8 * E, i0 + 16 * E, i0 + 8 * (2 * E + U)
        a.sort_ws, a.sort_ws_bytes, a.status = ws['sort'].data_ptr(), ws['sort'].numel(), ws['status'].data_ptr()
        a.out = out.data_ptr()
        _native.check(lib.tgmx_ctan_forward(a, _native.stream_ptr()), 'tgmx_ctan_forward')
        return out, saved

    def check(self) -> None:
        """Raise if a forward saw an ``edge_index`` entry outside ``[0, U)`` (such entries are clamped on the device).  Reads the device."""
        ws = getattr(self, '_ws', None)
        if ws and ws.get('status') is not None and int(ws['status'].item()):
            ws['status'].zero_()
            raise ValueError('CTAN: edge_index held node positions outside [0, node_x.shape[0])')


class CTANMemory(TransientCaches, nn.Module):
    """The CTAN Memory model.

    Args:
        num_nodes (int): The number of nodes to save memories for.
        memory_dim (int): The hidden memory dimensionality.
        aggr_module (Callable): The message aggregator function which aggregates messages to the same destination into a single
            representation: this package's ``LastAggregator`` (native) or ``MeanAggregator`` (composed from torch ops).
        init_time (int): Start time of the graph, used during memory reset.
    """

    _TRANSIENT = ('_scratch',)

    def __init__(self, num_nodes: int, memory_dim: int, aggr_module: Callable, init_time: int = 0) -> None:
        super().__init__()
        if not isinstance(aggr_module, (LastAggregator, MeanAggregator)):
            raise NotImplementedError(f'CTANMemory: aggr_module {type(aggr_module).__name__} is not supported (LastAggregator, MeanAggregator)')
        self.num_nodes = num_nodes
        self.memory_dim = memory_dim
        self.init_time = init_time
        self.aggr_module = aggr_module
        self.register_buffer('memory', torch.zeros(num_nodes, memory_dim))
        self.register_buffer('last_update', torch.ones(self.num_nodes, dtype=torch.long) * init_time)
        self.register_buffer('_assoc', torch.empty(num_nodes, dtype=torch.long))

    def reset_parameters(self) -> None:
        if hasattr(self.aggr_module, 'reset_parameters'):
            self.aggr_module.reset_parameters()
        self.reset_state()

    def reset_state(self) -> None:
        self.memory.data.fill_(0)
        self.last_update.fill_(self.init_time)

    def detach(self) -> None:
        self.memory.detach_()

    def forward(self, n_id: Tensor) -> Tuple[Tensor, Tensor]:
        _native.require_device(self.memory, 'CTANMemory: memory')
        return self.memory[n_id], self.last_update[n_id]

    def _tables(self) -> Tuple[Tensor, Tensor, Tensor]:
        """The per-node scratch of the native update at its rest values (the update leaves it so) and the status word."""
        dev = self.memory.device
        s = getattr(self, '_scratch', None)
        if s is None or s[0].device != dev or s[0].numel() != self.num_nodes:
            s = self._scratch = (torch.zeros(self.num_nodes, dtype=torch.int64, device=dev),
                                 torch.full((self.num_nodes,), _INT64_MIN, dtype=torch.int64, device=dev),
                                 torch.zeros(1, dtype=torch.int32, device=dev))  # fmt: skip
        return s

    def update_state(self, src: Tensor, pos_dst: Tensor, t: Tensor, src_emb: Tensor, pos_dst_emb: Tensor) -> None:
        """memory / last_update of every node in ``cat[src, pos_dst]`` from row p of ``cat[src_emb, pos_dst_emb]`` (the embeddings may
        hold more rows than ``src``, as the reference's evaluation loop passes them)."""
        _native.require_device(self.memory, 'CTANMemory: memory')
        for name, v in (('src', src), ('pos_dst', pos_dst), ('t', t), ('src_emb', src_emb), ('pos_dst_emb', pos_dst_emb)):
            _native.require_device(v, f'CTANMemory.update_state: {name}')
        B = src.numel()
        if pos_dst.numel() != B or t.numel() != B:
            raise ValueError(f'CTANMemory.update_state: src, pos_dst, t hold {B}, {pos_dst.numel()}, {t.numel()} entries')
        if src_emb.shape[0] + pos_dst_emb.shape[0] < 2 * B or src_emb.shape[-1] != self.memory_dim or pos_dst_emb.shape[-1] != self.memory_dim:
            raise ValueError(f'CTANMemory.update_state: embeddings {tuple(src_emb.shape)} and {tuple(pos_dst_emb.shape)} for {B} events, '
                             f'memory_dim {self.memory_dim}')  # fmt: skip
        if B == 0:
            return
        if isinstance(self.aggr_module, MeanAggregator):
            return self._update_state_composed(src, pos_dst, t, src_emb, pos_dst_emb)
        if self.memory.dtype != torch.float32:
            raise NotImplementedError('CTANMemory: the native update takes a float32 memory')
        ids = lambda v: v.contiguous() if v.dtype in (torch.int32, torch.int64) else v.long().contiguous()
        s, d = ids(src), ids(pos_dst)
        t64 = t.to(torch.int64).contiguous()
        se, de = _ops._f32c(src_emb.detach(), 'src_emb'), _ops._f32c(pos_dst_emb.detach(), 'pos_dst_emb')
        key, tmax, status = self._tables()
        lib = _native.load()
        _native.check(
            lib.tgmx_ctan_memory_update(s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64, t64.data_ptr(), B, se.data_ptr(),
                                        de.data_ptr(), se.shape[0], self.memory_dim, self.num_nodes, self.memory.data_ptr(),
                                        self.last_update.data_ptr(), key.data_ptr(), tmax.data_ptr(), status.data_ptr(),
                                        _native.stream_ptr(self.memory.device.index)),
            'tgmx_ctan_memory_update',
        )  # fmt: skip

    def _update_state_composed(self, src: Tensor, pos_dst: Tensor, t: Tensor, src_emb: Tensor, pos_dst_emb: Tensor, last: bool = False) -> None:
        """The reference's update_state from torch ops on the device (``unique`` synchronises with the host): MeanAggregator's path, and with
        ``last=True`` what the native LastAggregator update is timed against."""
        idx = torch.cat([src, pos_dst], dim=0).long()
        _idx = idx.unique()
        n = _idx.size(0)
        self._assoc[_idx] = torch.arange(n, device=_idx.device)
        local = self._assoc[idx]
        t = torch.cat([t, t], dim=0)
        emb = torch.cat([src_emb, pos_dst_emb], dim=0).detach()
        last_update = torch.full((n,), _INT64_MIN, dtype=t.dtype, device=t.device).scatter_reduce(0, local, t, 'amax')
        if last:
            scores = torch.full((n, t.size(0)), float('-inf'), device=t.device)
            scores[local, torch.arange(t.size(0), device=t.device)] = t.float()
            aggr = emb[scores.argmax(dim=1)]
        else:
            rows = emb[: idx.numel()]
            aggr = torch.zeros((n, rows.shape[1]), dtype=rows.dtype, device=rows.device).index_add_(0, local, rows)
            cnt = torch.zeros(n, dtype=rows.dtype, device=rows.device).index_add_(0, local, torch.ones_like(local, dtype=rows.dtype))
            aggr = aggr / cnt.clamp(min=1).unsqueeze(-1)
        self.last_update[_idx] = last_update
        self.memory[_idx] = aggr.to(self.memory.dtype)

    def check(self) -> None:
        """Raise if an ``update_state`` saw a node id outside ``[0, num_nodes)`` (such positions are skipped).  Reads the device."""
        s = getattr(self, '_scratch', None)
        if s is not None and int(s[2].item()):
            s[2].zero_()
            raise ValueError('CTANMemory: update_state saw node ids outside [0, num_nodes)')
