"""``TimeGapNeighborHook`` -- the one-hop "time-gap" neighbours GraphMixer's node encoder averages (the reference keeps this hook in its
example, examples/linkproppred/graphmixer.py: ``GraphMixerHook``).

For a batch over global events ``[start_idx, end_idx)`` the window is the edges whose event index lies in ``[lb, ub)``, both clamped into
``[max(end_idx - time_gap, 0), end_idx]`` as ``EdgeStore.event_range`` does: ``ub`` is the first event after time ``min(edge_time) - 1``
(edges tied with the batch's first timestamp are left out), ``lb`` the first event at the view's carried ``start_time``.  ``time_gap``
counts events, node events included, and ``end_idx`` is the batch's NOMINAL end (slice start + batch size, also for the last, partial
batch).  Every window edge ``(u, v)`` makes ``v`` a neighbour of ``u`` and ``u`` one of ``v`` (a self loop twice), in stream order.

Outputs (int32, on the device; no device -> host read -- every size is known on the host):

* ``time_gap_nbr`` [2 W]: the window's incidences grouped by node id, each node's neighbours in stream order;
* ``time_gap_lo`` / ``time_gap_cnt`` [S]: the run ``time_gap_nbr[lo : lo + cnt]`` of seed ``i`` of ``cat(edge_src, edge_dst, neg)``
  -- the example's ``time_gap_nbrs[i]`` list.
"""
from __future__ import annotations

import torch

from .. import _native
from ..core import DGBatch, DGraph
from ..core.store import SliceBounds
from .base import StatelessHook
from .registry import hook


@hook
class TimeGapNeighborHook(StatelessHook):
    """Materialize the neighbours of every seed within the last ``time_gap`` events before the batch (GraphMixer's node encoder input).

    Key words: time gap, GraphMixer, one-hop window.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time', 'neg'}
    _cls_produces = {'time_gap_nbr', 'time_gap_lo', 'time_gap_cnt'}

    def __init__(self, time_gap: int) -> None:
        super().__init__()
        if isinstance(time_gap, bool) or not isinstance(time_gap, int):
            raise ValueError(f'time_gap must be an int, got {type(time_gap).__name__}')
        if time_gap < 0:
            raise ValueError(f'time_gap must be >= 0, got {time_gap}')
        self.time_gap = time_gap
        self._ws = None
        self.__post_init__()

    def window(self, dg: DGraph) -> tuple:
        """The window's edge range ``[lo, hi)`` in the store (host integers) for the batch view ``dg``."""
        sl = dg._slice
        if sl.end_idx is None:
            raise ValueError('TimeGapNeighborHook needs event-ordered batches (batch_unit="r"): a time-unit batch has no end event index '
                             'to count the time gap back from')
        st = dg._storage
        lo, hi = dg._edge_range
        if hi <= lo:
            return 0, 0
        first_time = int(st._time_np[st._edge_pos_np[lo]])  # the store is time-sorted: the batch's first edge holds min(edge_time)
        win = SliceBounds(start_time=sl.start_time, end_time=first_time - 1, start_idx=max(sl.end_idx - self.time_gap, 0), end_idx=sl.end_idx)
        w_lo, w_hi = st.edge_range(win)
        return w_lo, max(w_lo, w_hi)

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        neg = getattr(batch, 'neg', None)
        if neg is None:
            raise ValueError('TimeGapNeighborHook requires batch.neg (register a negative sampler before it)')
        for name, t in (('edge_src', batch.edge_src), ('edge_dst', batch.edge_dst), ('neg', neg)):
            _native.require_device(t, f'batch.{name}')
        w_lo, w_hi = self.window(dg)
        W = w_hi - w_lo
        device = batch.edge_src.device
        arr = dg._storage.on(device)
        lib = _native.load()
        seeds = [t if (t.dtype == torch.int32 and t.is_contiguous()) else t.to(torch.int32).contiguous() for t in (batch.edge_src, batch.edge_dst, neg)]
        S = sum(t.numel() for t in seeds)
        nbr = torch.empty(2 * W, dtype=torch.int32, device=device)
        lo_cnt = torch.empty((2, S), dtype=torch.int32, device=device)
        ws_ptr, ws_bytes = 0, 0
        if W > 0:
            need = int(lib.tgmx_time_gap_workspace_bytes(W))
            ws = self._ws
            if ws is None or ws.device != device or ws.numel() < need:
                ws = self._ws = torch.empty(max(need, 2 * (0 if ws is None else ws.numel())), dtype=torch.uint8, device=device)
            ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
        _native.check(
            lib.tgmx_time_gap_group(arr.src.data_ptr(), arr.dst.data_ptr(), w_lo, W, seeds[0].data_ptr(), seeds[0].numel(), seeds[1].data_ptr(),
                                    seeds[1].numel(), seeds[2].data_ptr(), seeds[2].numel(), ws_ptr, ws_bytes, nbr.data_ptr(),
                                    lo_cnt[0].data_ptr(), lo_cnt[1].data_ptr(), _native.stream_ptr(device.index)),
            'tgmx_time_gap_group',
        )  # fmt: skip
        self.add_batch_attribute(batch, 'time_gap_nbr', nbr)
        self.add_batch_attribute(batch, 'time_gap_lo', lo_cnt[0])
        self.add_batch_attribute(batch, 'time_gap_cnt', lo_cnt[1])
        return batch

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_ws'] = None
        return state
