"""``batch.neg_batch_list`` as the TGB negative-sampler hooks produce it: a plain list of one int32 tensor per positive edge, as the
reference's, that also keeps the padded matrix its entries are views of, so a one-vs-many decoder can take ``B`` equally long rows as one
``[B, Q]`` tensor instead of concatenating ``B`` of them."""
from __future__ import annotations

from typing import List, Optional

import torch


class NegBatchList(list):
    """``list`` of ``matrix[b, :lengths[b]]``.

    Attributes:
        matrix: ``[B, Qpad]`` int32, ``-1`` behind every row's ids.
        lengths: ``[B]`` int32, on the matrix's device.
        uniform: the rows' common length, or ``None`` when they differ (or there are none).
    """

    matrix: torch.Tensor
    lengths: torch.Tensor
    uniform: Optional[int]

    def __init__(self, matrix: torch.Tensor, lengths: torch.Tensor, host_lengths: List[int]) -> None:
        super().__init__(matrix[b, :n] for b, n in enumerate(host_lengths))
        self.matrix, self.lengths = matrix, lengths
        self.uniform = host_lengths[0] if host_lengths and min(host_lengths) == max(host_lengths) else None

    def as_matrix(self) -> Optional[torch.Tensor]:
        """``[B, Q]`` when every row has ``Q`` ids, else ``None``."""
        return None if self.uniform is None else self.matrix[:, : self.uniform]


def uniform_matrix(negatives) -> Optional[torch.Tensor]:
    """What a ``query_one_vs_many`` may read instead of ``B`` tensors: the matrix of an untouched :class:`NegBatchList` of equal rows."""
    if type(negatives) is NegBatchList and len(negatives) == negatives.matrix.shape[0]:
        return negatives.as_matrix()
    return None
