"""``GraphPredictor`` (tgm/nn/decoder/graphproppred.py) on HIP kernels: same constructor, ``self.graph_pooling`` / ``self.model`` and
``state_dict`` keys.

Without gradients on the device, ``MeanEmbdPooling`` / ``SumEmbdPooling`` over ``z_nodes [N, in_dim]`` and the MLP over the pooled row are
one native call (``tgmx_decoder_forward``): the pooling adds the rows in a fixed order (``tgmx_pool_rows``: chunks of 128 rows, then the
chunks), so two runs give the same bits.  Any other :class:`Aggregator` pools in torch and the MLP after it runs natively.  With gradients,
on the host or outside the native envelope it is the same arithmetic as torch ops.  The output is ``[out_dim]``, as the reference's
``squeeze`` leaves it."""
from __future__ import annotations

from typing import Optional

import torch.nn as nn
from torch import Tensor

from .. import _native
from ._decoder_head import DecoderHead, build_mlp, linears
from .aggregation import Aggregator, MeanEmbdPooling, SumEmbdPooling, require_aggregator

_POOL_MAX_DIM = 1536  # tgmx_pool_rows keeps four partial rows of doubles in LDS


class GraphPredictor(DecoderHead, nn.Module):
    """``model(graph_pooling(z_nodes))``: ``graph_pooling`` is an :class:`Aggregator`, ``MeanEmbdPooling(in_dim)`` by default."""

    def __init__(self, in_dim: int, out_dim: int = 1, nlayers: int = 2, hidden_dim: int = 64, graph_pooling: Optional[Aggregator] = None) -> None:
        super().__init__()
        self.model = build_mlp(in_dim, hidden_dim, out_dim, nlayers)
        self.graph_pooling = MeanEmbdPooling(dim=in_dim) if graph_pooling is None else graph_pooling
        require_aggregator(self.graph_pooling)

    def forward(self, z_nodes: Tensor) -> Tensor:
        if not (self._native_ok(z_nodes) and len(linears(self.model)) <= _native.DECODER_MAX_LAYERS):
            return self.model(self.graph_pooling(z_nodes))
        kind = {MeanEmbdPooling: 'mean', SumEmbdPooling: 'sum'}.get(type(self.graph_pooling))
        D = self.model[0].in_features
        if kind is None or z_nodes.dim() != 2 or z_nodes.shape[0] == 0 or z_nodes.shape[1] != D or not 1 < D <= _POOL_MAX_DIM:
            pooled = self.graph_pooling(z_nodes)
            if pooled.dim() < 1 or pooled.shape[-1] != D:
                return self.model(pooled)
            return self._mlp_rows(pooled.reshape(-1, D).contiguous()).view(*pooled.shape[:-1], -1)
        x = z_nodes.contiguous()
        N = x.shape[0]

        def fill(a, w):
            a.a1, a.lda1, a.n1 = x.data_ptr(), x.stride(0), N
            return x

        nws = _native.load().tgmx_pool_rows_scratch_floats(N, D)
        return self._run('rows', 1, fill, x.device, pool=kind, scratch=(0, D, nws)).view(-1)
