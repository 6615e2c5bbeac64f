"""``NodePredictor`` (tgm/nn/decoder/nodeproppred.py) on HIP kernels: same constructor, ``self.model`` and ``state_dict`` keys.

Without gradients on the device the MLP is one native call (``tgmx_decoder_forward``, rows form): the hidden layers are exact-fp32 MFMA
GEMMs with the ReLU in their epilogue, a last layer of at most 16 outputs is a row dot.  With gradients to track it is the same layer chain
as a ``torch.autograd.Function`` (``_decoder_train.py``: one native call forward, one back).  On the host or outside the native envelope
it is the same arithmetic as torch ops."""
from __future__ import annotations

import torch.nn as nn
from torch import Tensor

from .. import _native
from ._decoder_head import DecoderHead, build_mlp, linears


class NodePredictor(DecoderHead, nn.Module):
    """An MLP over node embeddings ``[..., in_dim] -> [..., out_dim]`` (``nlayers = 1`` builds the two Linears of ``nlayers = 2``)."""

    def __init__(self, in_dim: int, out_dim: int = 1, nlayers: int = 2, hidden_dim: int = 64) -> None:
        super().__init__()
        self.model = build_mlp(in_dim, hidden_dim, out_dim, nlayers)

    def forward(self, z_node: Tensor) -> Tensor:
        if z_node.dim() >= 1 and z_node.numel() > 0 and self._trainable(z_node) and z_node.shape[-1] == self.model[0].in_features:
            x = z_node.reshape(-1, z_node.shape[-1]).contiguous()  # gradients to track: the saving forward, one native call back
            return self._train('rows', None, (*z_node.shape[:-1], -1), x)
        if not (z_node.dim() >= 1 and self._native_ok(z_node) and len(linears(self.model)) <= _native.DECODER_MAX_LAYERS
                and z_node.shape[-1] == self.model[0].in_features):  # fmt: skip
            return self.model(z_node)
        x = z_node.reshape(-1, z_node.shape[-1]).contiguous()
        return self._mlp_rows(x).view(*z_node.shape[:-1], -1)
