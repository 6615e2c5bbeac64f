"""BatchAnalyticsHook (contract of tgm/hooks/analytics/batch_analytics.py): seven statistics of one batch.

    num_edge_events, num_node_events   element counts of edge_src / node_x_nids (None counts 0)
    num_unique_nodes                   distinct ids over edge_src u edge_dst u node_x_nids
    avg_degree                         0.0 without edges, else the float32 quotient float32(2 E) / float32(U_edge), U_edge = distinct ids over
                                       edge_src u edge_dst (E = 7, U_edge = 6 gives 2.3333332538604736)
    num_repeated_edge_events           E - distinct (src, dst, time) triples, the time at full int64 width; 0 without edge_time
    num_repeated_node_events           Nn - distinct (nid, time) pairs; 0 without node_x_time
    num_unique_timestamps              distinct values over edge_time u node_x_time.  When exactly ONE of the two is None the reference
                                       concatenates with an empty float32 tensor, so the times are rounded to float32 before they are counted
                                       ([2**24, 2**24 + 1, 5] counts 2); with both present the count is exact.  Kept.

The reference makes seven ``torch.unique`` + ``.item()`` round trips.  On a ROCm device a batch is one ``tgmx_batch_analytics`` call
(csrc/analytics.hip: five batch-local hash sets) writing eight words, read back once -- or, with ``sync=False`` (extension), not at all: the
seven attributes are then 0-d device tensors, views of that one buffer (int64 counts, float32 ``avg_degree``).  Host tensors run the same
definition over numpy.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from ... import _native
from ...core import DGBatch, DGraph
from ..base import StatelessHook
from ..registry import hook

_INT = (torch.int32, torch.int64)
# word of the output buffer behind each attribute (avg_degree: the float32 at the start of word 4)
_WORD = dict(num_edge_events=0, num_node_events=1, num_unique_timestamps=2, num_unique_nodes=3, num_repeated_edge_events=5, num_repeated_node_events=6)
_ORDER = ('num_edge_events', 'num_node_events', 'num_unique_timestamps', 'num_unique_nodes', 'avg_degree', 'num_repeated_edge_events',
          'num_repeated_node_events')  # fmt: skip


def _native_vector(t: Optional[torch.Tensor], what: str) -> Optional[torch.Tensor]:
    """An id or time vector as the kernels read it (contiguous int32 / int64); other integer dtypes are widened."""
    if t is None:
        return None
    if t.dtype not in _INT:
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError(f'{what} must be an integer tensor on the device path, got {t.dtype}')
        t = t.to(torch.int64)
    return t.contiguous().view(-1)


def require_on(device: torch.device, who: str, **tensors: Optional[torch.Tensor]) -> None:
    """Every tensor given lives on ``device``: a kernel is handed raw pointers, so a field left elsewhere must stop here."""
    for name, t in tensors.items():
        if t is not None and t.device != device:
            raise ValueError(f'{who}: {name} is on {t.device}, the other fields on {device}')


def an_batch(src, dst, edge_time, nids, node_time) -> '_native.AnBatch':
    """tgmx_an_batch_t over tensors already passed through ``_native_vector`` (the caller keeps them alive)."""
    b = _native.AnBatch()
    n = lambda t: 0 if t is None else int(t.numel())
    is64 = lambda t: int(t is not None and t.dtype == torch.int64)
    ptr = lambda t: t.data_ptr() if n(t) else None
    b.src, b.dst, b.E, b.src_is64, b.dst_is64 = ptr(src), ptr(dst), n(src), is64(src), is64(dst)
    b.edge_time, b.Et, b.edge_time_is64 = ptr(edge_time), n(edge_time), is64(edge_time)
    b.nids, b.Nn, b.nids_is64 = ptr(nids), n(nids), is64(nids)
    b.node_time, b.Nt, b.node_time_is64 = ptr(node_time), n(node_time), is64(node_time)
    return b


@hook
class BatchAnalyticsHook(StatelessHook):
    """Compute simple batch-level statistics.  ``sync=False`` (extension): 0-d tensors on the batch's device instead of Python numbers,
    nothing read back.

    Key words: global statistics, degree, number of events and repeated events.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time', 'node_x_time', 'node_x_nids'}
    _cls_produces = {'num_edge_events', 'num_node_events', 'num_unique_timestamps', 'num_unique_nodes', 'avg_degree', 'num_repeated_edge_events',
                     'num_repeated_node_events'}  # fmt: skip

    def __init__(self, id: Optional[str] = None, sync: bool = True) -> None:
        super().__init__()
        self._id = id
        self.sync = bool(sync)
        self._ws: Optional[torch.Tensor] = None
        self.__post_init__()

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        fields = (batch.edge_src, batch.edge_dst, batch.edge_time, getattr(batch, 'node_x_nids', None), getattr(batch, 'node_x_time', None))
        device = next((t.device for t in fields if t is not None), torch.device('cpu'))
        out = self._count_device(fields, device) if device.type == 'cuda' else self._count_host(fields)
        if self.sync:
            w = out.tolist()  # the one read of the batch
            E, u_edge = w[0], w[7]
            values = {k: w[i] for k, i in _WORD.items()}
            values['avg_degree'] = float(np.float32(2 * E) / np.float32(u_edge)) if u_edge else 0.0
        else:
            values = {k: out[i] for k, i in _WORD.items()}
            values['avg_degree'] = out.view(torch.float32)[8]
        for k in _ORDER:
            self.add_batch_attribute(batch, k, values[k])
        return batch

    def _count_device(self, fields, device: torch.device) -> torch.Tensor:
        src, dst, et, nids, nt = fields
        if (src is None) != (dst is None):
            raise ValueError('BatchAnalyticsHook on the device needs edge_src and edge_dst together')
        names = ('edge_src', 'edge_dst', 'edge_time', 'node_x_nids', 'node_x_time')
        require_on(device, 'BatchAnalyticsHook', **dict(zip(names, fields)))
        src, dst, et, nids, nt = (_native_vector(t, n) for t, n in zip(fields, names))
        b = an_batch(src, dst, et, nids, nt)
        if (b.E and src.numel() != dst.numel()) or (et is not None and b.Et != b.E) or (nt is not None and nids is not None and b.Nt != b.Nn):
            raise ValueError(f'BatchAnalyticsHook: field lengths differ (edges {b.E}, edge times {b.Et}, node events {b.Nn}, node times {b.Nt})')
        lib = _native.load()
        nbytes = int(lib.tgmx_batch_analytics_workspace_bytes(b.E, b.Et, b.Nn, b.Nt))
        if nbytes == 0:
            raise ValueError(f'BatchAnalyticsHook: sizes beyond the kernel (edges {b.E}, node events {b.Nn}; below 2^28 each)')
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        out = torch.empty(8, dtype=torch.int64, device=device)
        rc = lib.tgmx_batch_analytics(ctypes.byref(b), int((fields[2] is None) != (fields[4] is None)), out.data_ptr(), self._ws.data_ptr(),
                                      self._ws.numel(), _native.stream_ptr(device.index))  # fmt: skip
        if rc:
            _native.check(rc, 'tgmx_batch_analytics')
        return out

    @staticmethod
    def _count_host(fields) -> torch.Tensor:
        """The eight words ``tgmx_batch_analytics`` writes, over numpy."""
        src, dst, et, nids, nt = (None if t is None else t.detach().numpy().reshape(-1) for t in fields)
        wide = lambda parts: np.concatenate([p.astype(np.int64) for p in parts]) if parts else np.empty(0, dtype=np.int64)
        distinct = lambda parts: int(np.unique(wide([p for p in parts if p is not None])).size)
        distinct_rows = lambda cols: int(np.unique(np.stack([c.astype(np.int64) for c in cols], 1), axis=0).shape[0])
        E = 0 if src is None else int(src.size)
        Nn = 0 if nids is None else int(nids.size)
        times = wide([t for t in (et, nt) if t is not None])
        if (et is None) != (nt is None):
            times = times.astype(np.float32)
        has_edges = src is not None and dst is not None and E > 0
        u_edge = distinct([src, dst]) if has_edges else 0
        rep_e = E - distinct_rows([src, dst, et]) if has_edges and et is not None else 0
        rep_n = Nn - distinct_rows([nids, nt]) if Nn > 0 and nt is not None else 0
        out = torch.zeros(8, dtype=torch.int64)
        out[0], out[1], out[2], out[3], out[5], out[6], out[7] = E, Nn, int(np.unique(times).size), distinct([src, dst, nids]), rep_e, rep_n, u_edge
        out.view(torch.float32)[8] = float(np.float32(2 * E) / np.float32(u_edge)) if has_edges else 0.0
        return out
