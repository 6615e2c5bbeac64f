"""The merge and pooling operators of the decoders (tgm/nn/modules/aggregation.py): same names, constructors and ``state_dict`` keys.

These objects only DESCRIBE the operation: called directly they are a line of torch (any device, any dtype -- ``ConcatMerge`` passes integer
tensors through ``torch.cat`` unchanged).  ``LinkPredictor`` / ``GraphPredictor`` recognise the four shipped here and run them inside
their native head (csrc/decoder.hip) instead of calling them; any other object that satisfies :class:`Aggregator` is called as it is.
"""
from __future__ import annotations

from typing import Protocol, runtime_checkable

import torch
import torch.nn as nn
from torch import Tensor


@runtime_checkable
class Aggregator(Protocol):
    """What a decoder asks of a merge / pooling object: ``out_channels`` (the width it returns) and a call on embedding tensors."""

    @property
    def out_channels(self) -> int: ...

    def __call__(self, *args: Tensor, **kwargs: Tensor) -> Tensor: ...


class ConcatMerge:
    """``[z_src | z_dst]``: two ``[N, dim]`` embeddings side by side, ``[N, 2 dim]``."""

    def __init__(self, dim: int) -> None:
        self.dim = dim

    @property
    def out_channels(self) -> int:
        return 2 * self.dim

    def __call__(self, z_src: Tensor, z_dst: Tensor) -> Tensor:
        return torch.cat((z_src, z_dst), dim=1)


class LearnableSumMerge(nn.Module):
    """``lin_src(z_src) + lin_dst(z_dst)``, both ``Linear(dim, dim)``: ``[N, dim]``."""

    def __init__(self, dim: int) -> None:
        super().__init__()
        self.dim = dim
        self.lin_src = nn.Linear(dim, dim)
        self.lin_dst = nn.Linear(dim, dim)

    @property
    def out_channels(self) -> int:
        return self.dim

    def __call__(self, z_src: Tensor, z_dst: Tensor) -> Tensor:
        return self.lin_src(z_src) + self.lin_dst(z_dst)


class MeanEmbdPooling:
    """The column mean of ``[N, dim]`` node embeddings: ``[dim]``."""

    def __init__(self, dim: int) -> None:
        self.dim = dim

    @property
    def out_channels(self) -> int:
        return self.dim

    def __call__(self, z: Tensor) -> Tensor:
        return z.mean(dim=0).squeeze()


class SumEmbdPooling:
    """The column sum of ``[N, dim]`` node embeddings: ``[dim]``."""

    def __init__(self, dim: int) -> None:
        self.dim = dim

    @property
    def out_channels(self) -> int:
        return self.dim

    def __call__(self, z: Tensor) -> Tensor:
        return z.sum(dim=0).squeeze()


def require_aggregator(obj: object) -> None:
    from ..exceptions import BadAggregatorProtocolError

    if not isinstance(obj, Aggregator):
        raise BadAggregatorProtocolError(
            f'Cannot validate {type(obj).__name__}: must implement __call__(*args: torch.Tensor, **kwargs: torch.Tensor) -> torch.Tensor and out_channels() -> int'
        )
