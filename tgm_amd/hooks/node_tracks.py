"""EdgeEventsSeenNodesTrackHook (contract of tgm/hooks/node_tracks.py): of the nodes labelled in a batch, those an edge event has brought so far.

Per batch: every id of ``edge_src`` and ``edge_dst`` is marked first; then ``batch_nodes_mask`` = the int64 positions of ``node_y_nids`` whose node
is marked (a node first met in this very batch counts), ``seen_nodes`` = the ids there, in ``node_y_nids``' dtype, repeats kept.  Without labels
both are empty (``seen_nodes`` int32) and the marking still happens.  The nodeproppred scripts of DyGFormer and TPNet index with them:
``z[batch.seen_nodes]``, ``y[batch.batch_nodes_mask]``.

On a ROCm device a batch is one ``tgmx_seen_nodes_step`` call (csrc/analytics.hip: byte stores into the mask, then an ordered compaction by
one workgroup) and ONE read of {count, status} -- the outputs' length depends on the data.  Host tensors run the same definition with torch.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from ..core import DGBatch, DGraph
from .analytics.batch_analytics import _native_vector, require_on
from .base import StatefulHook
from .registry import hook


@hook
class EdgeEventsSeenNodesTrackHook(StatefulHook):
    """Return the nodes among the current batch's node labels that past (or this batch's) edge events have brought.

    Args:
        num_nodes (int): Total number of nodes to track.
        id (str): A unique identifier for the hook. The hook's name and all attributes it produces are suffixed with it.

    Raises:
        ValueError: If ``num_nodes`` is negative.

    Key words: node appearance, node property prediction, nodeproppred.
    """

    _cls_requires = {'edge_src', 'edge_dst'}
    _cls_produces = {'seen_nodes', 'batch_nodes_mask'}

    def __init__(self, num_nodes: int, id: Optional[str] = None) -> None:
        super().__init__()
        if num_nodes < 0:
            raise ValueError('num_nodes must be non-negative')
        self._seen_mask = torch.zeros(num_nodes, dtype=torch.bool)
        self._device = torch.device('cpu')
        self._state: Optional[torch.Tensor] = None  # device path: int64 {count, status}
        self._status = 0  # status bits read back and not yet reported
        self._id = id
        self.__post_init__()

    def reset_state(self) -> None:
        self._seen_mask.fill_(False)

    def check(self) -> None:
        """Raise ``ValueError`` (once) if an id outside ``[0, num_nodes)`` was offered on the device since the last check: it was not
        marked and not reported as seen.  One device-to-host read.  (Host tensors raise ``IndexError`` at the call, as the reference does.)"""
        if self._state is not None:
            bits = int(self._state[1])
            if bits:
                self._state[1:].zero_()
            self._status |= bits
        bits, self._status = self._status, 0
        if bits & _native.AN_BAD_ID:
            raise ValueError(f'EdgeEventsSeenNodesTrackHook: ids must lie in [0, {self._seen_mask.numel()}); an id outside was offered')

    def _move_to_device_if_needed(self, device: torch.device) -> None:
        if device != self._device:
            self._device = device
            self._seen_mask = self._seen_mask.to(device)
            self._state = None

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        self._move_to_device_if_needed(dg.device)  # no-op after the first batch
        nids = batch.node_y_nids
        step = self._step_device if self._seen_mask.device.type == 'cuda' else self._step_host
        pos, seen = step(batch.edge_src, batch.edge_dst, nids)
        self.add_batch_attribute(batch, 'batch_nodes_mask', pos)
        self.add_batch_attribute(batch, 'seen_nodes', seen)
        return batch

    def _step_host(self, src, dst, nids):
        self._seen_mask[torch.cat([src, dst]).long()] = True
        if nids is None:
            nids = torch.empty(0, dtype=torch.int32, device=self._seen_mask.device)
        hit = self._seen_mask[nids.long()]
        return torch.nonzero(hit, as_tuple=True)[0], nids[hit]

    def _step_device(self, src, dst, nids):
        device = self._seen_mask.device
        require_on(device, 'EdgeEventsSeenNodesTrackHook', edge_src=src, edge_dst=dst, node_y_nids=nids)
        src, dst = (_native_vector(t, n) for t, n in ((src, 'edge_src'), (dst, 'edge_dst')))
        if src.shape[0] != dst.shape[0]:
            raise ValueError(f'edge_src has {src.shape[0]} entries, edge_dst {dst.shape[0]}')
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.int64, device=device)
        Ny = 0 if nids is None else int(nids.shape[0])
        if Ny:
            if nids.dtype not in (torch.int32, torch.int64):  # seen_nodes answers in this dtype: nothing to widen to
                raise TypeError(f'node_y_nids must be an int32 or int64 tensor on the device path, got {nids.dtype}')
            nids = nids.contiguous()
            pos = torch.empty(Ny, dtype=torch.int64, device=device)
            ids = torch.empty_like(nids)
        rc = _native.load().tgmx_seen_nodes_step(self._seen_mask.data_ptr(), self._seen_mask.numel(), src.data_ptr(), int(src.dtype == torch.int64),
                                                 dst.data_ptr(), int(dst.dtype == torch.int64), src.shape[0], nids.data_ptr() if Ny else 0,
                                                 int(Ny and nids.dtype == torch.int64), Ny, pos.data_ptr() if Ny else 0, ids.data_ptr() if Ny else 0,
                                                 self._state.data_ptr(), _native.stream_ptr(device.index))  # fmt: skip
        if rc:
            _native.check(rc, 'tgmx_seen_nodes_step')
        if not Ny:  # nothing to compact, nothing to read: the marking's status waits for the next read
            empty = torch.empty(0, dtype=torch.int32 if nids is None else nids.dtype, device=device)
            return torch.empty(0, dtype=torch.int64, device=device), empty
        count, bits = self._state.tolist()  # the one read of the batch
        if bits:
            self._state[1:].zero_()
            self._status |= bits
        return pos[:count], ids[:count]
