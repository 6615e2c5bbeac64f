"""PopTrackPredictor (the reference's ``tgm/nn/modules/poptrack.py``) with its popularity vector on the device.

Composed, not native: ``update`` is an integer ``index_add_`` (the occurrences of every node), ``add_`` once per round of occurrences and
``mul_``, a query is one gather, all torch ops on device tensors.  Nothing here is a hot path, so there is no kernel of this project's behind
it.  Per node an update adds ``1.0f`` once per occurrence as a destination, one after the other as the reference's host loop does, and then
multiplies by ``f32(decay)`` (a 0-dim float32 tensor on the device).  ``update`` reads one integer back (the number of rounds).

Cost: ``update`` reads one integer back (the number of rounds) and issues two small launches per round, and the rounds of a call are the
most occurrences of ONE destination in it: a handful for a loader batch, but as many as the call has events when they all share a
destination (a constructor handed 100 000 events of a popular node takes that many rounds).  Exactness was put first; offer a long stream
in pieces where that matters.

The reference's argument checks, their order and their messages are kept.  Queries need integer ids: float ids raise ``IndexError``, as the
reference's indexing does.  ``k`` and ``query_src`` are otherwise unused, as in the reference.
"""
from __future__ import annotations

import torch

from .. import _native
from .edgebank import EdgeBankPredictor


class PopTrackPredictor:
    def __init__(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor, num_nodes: int, k: int = 50, decay: float = 0.9) -> None:
        """The PopTrack baseline (https://openreview.net/pdf?id=9kLDrE5rsW): an edge's score is the decayed popularity of its destination.

        Args:
            src, dst, ts: the edges the popularity starts with.
            num_nodes: number of nodes.
            k: number of popular nodes to retrieve from; validated (``0 < k <= num_nodes``) and otherwise unused, as in the reference.
            decay: what every update multiplies the popularity by, in ``(0, 1]``.
        """
        if 0 >= k:
            raise ValueError('K must be positive')
        if decay <= 0 or decay > 1:
            raise ValueError('Decay must be in (0,1]')
        if num_nodes <= 0:
            raise ValueError('``num_nodes`` must be set to the total number of nodes.')
        if k > num_nodes:
            raise ValueError('``k`` must be smaller than ``num_nodes``.')
        self._check_input_data(src, dst, ts)
        _native.require_device(dst, 'PopTrackPredictor: dst')
        self.popularity = torch.zeros(num_nodes, device=dst.device)
        self.k = k
        self.decay = decay
        # float32 on the device: the product below is then f32 x f32, as the reference's on the host (a Python scalar may be kept wider)
        self._decay = torch.full((), decay, dtype=torch.float32, device=dst.device)
        self.update(src, dst, ts)

    def update(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor) -> None:
        """One batch of edges: every destination's popularity += 1 per occurrence, then the whole vector *= decay."""
        self._check_input_data(src, dst, ts)
        _native.require_device(dst, 'PopTrackPredictor.update: dst')
        if dst.is_floating_point():
            dst = dst.long()  # floating tensors of integral values, as the other predictors take them
        # the reference's host index_add_ adds 1.0f once per occurrence, one after the other.  The device's index_add_ may add a node's
        # occurrences up first (lanes of a wave that share an address), which rounds differently where the popularity is no integer.  So
        # the occurrences are counted in integers, which is exact however they are combined, and added one round at a time.
        count = torch.zeros(self.popularity.shape, dtype=torch.int32, device=dst.device).index_add_(0, dst, torch.ones_like(dst, dtype=torch.int32))
        for done in range(int(count.max())):  # (one read from the device: the most occurrences of one node in the batch)
            self.popularity.add_((count > done).to(self.popularity.dtype))
        self.popularity.mul_(self._decay)

    def __call__(self, query_src: torch.Tensor, query_dst: torch.Tensor) -> torch.Tensor:
        """``popularity[query_dst]`` (float32); the source plays no part.  Integer ids only: float ids raise ``IndexError``."""
        _native.require_device(query_dst, 'PopTrackPredictor: query_dst')
        if query_dst.dtype not in (torch.int32, torch.int64):
            raise IndexError(f'tensors used as indices must be long, int, byte or bool tensors, got {query_dst.dtype}')
        return self.popularity[query_dst]

    _check_input_data = staticmethod(EdgeBankPredictor._check_input_data)
