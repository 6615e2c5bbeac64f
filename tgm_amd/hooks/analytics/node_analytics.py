"""NodeAnalyticsHook (contract of tgm/hooks/analytics/node_analytics.py): per-batch statistics of a set of tracked nodes, and of the batch's
edges and node events against what the stream has brought so far.

State.  Per tracked node: first and last time seen, the set of distinct times it appeared at, the set of its neighbours.  Global: the set of
distinct times, the set of directed (src, dst) pairs.

Per batch.  ``current_time`` = max(max edge_time, max node_x_time, 0).  The tracked nodes present -- tracked n distinct(edge_src, edge_dst,
node_x_nids) -- come first in ``node_stats``, ascending by id: ``first_seen`` is set once, ``last_seen = current_time``; ``appearances`` = size
of the node's time set after adding the times of the edges and node events it takes part in; ``degree`` = occurrences in cat(src, dst) (a self
loop counts 2); ``new_neighbors`` = neighbours of this batch not met before (a self loop makes the node its own neighbour); ``activity`` =
appearances / max(1, number of distinct times so far); ``lifetime`` = current_time - first_seen; ``time_since_last_seen`` = 0.0.  Then, in
``tracked_nodes`` order, the tracked nodes seen before but absent: degree 0, new_neighbors 0, lifetime = last - first, time_since_last_seen =
current_time - last (negative after an empty batch, whose current_time is 0: kept).  ``edge_stats``: ``new_edge_count`` = pairs not in the pair
set (a pair repeated inside the batch counts once), ``edge_novelty`` = new / E, ``edge_density`` = E / (U (U - 1)) with U = distinct(src u dst),
0.0 when U < 2; all zero without edges.  ``node_macro_stats``: computed after the per-node update, so ``new_node_count`` is the number of
``node_x_nids`` entries, with multiplicity, whose id is NOT tracked -- in every batch (kept) -- and ``node_novelty`` that count over Nn.
When edge_src, edge_dst and node_x_nids are all None: ``node_stats == {}``, the other two hold their zero defaults, and the three are written
WITHOUT the id suffix (kept).

The reference keeps all of this in Python dicts and sets, copies the batch to the host once per tracked node present and loops over every edge
in Python.  On a ROCm device the state lives there (csrc/analytics.hip: four pair tables over csrc/pairtable.h -- (src, dst); (tracked node,
neighbour); time -> dense id; (tracked node, time id) -- and per-node arrays), a batch is one ``tgmx_node_analytics_step`` call and ONE read of
a [T + 2, 8] integer block; the quotients are Python float divisions of those exact integers, so both paths give the same floats.  The
tables grow by ``grow_capacity``'s rule (nn/edgebank.py) from the occupancies that block brings back, before a call that could overflow.  The
device path takes integer times >= 0 and ids in [0, num_nodes): an event outside takes no part and :meth:`check` raises for it.  Host tensors
run the same definition over dicts and sets; there an id >= num_nodes raises ``IndexError`` as the reference's mask lookup does.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Set, Tuple

import torch
from torch import Tensor

from ... import _native
from ...core import DGBatch, DGraph
from ..base import StatefulHook
from ..registry import hook
from .batch_analytics import _native_vector, an_batch, require_on

_TABLES = ('edges', 'nbrs', 'times', 'apps')
_DEFAULT_CAPACITY = 1024


def _node_macro(count: int, Nn: int) -> Dict[str, Any]:
    return {'node_novelty': count / Nn if Nn else 0.0, 'new_node_count': count}


def _edge_stats(new: int, E: int, U: int) -> Dict[str, Any]:
    if not E:
        return {'edge_novelty': 0.0, 'edge_density': 0.0, 'new_edge_count': 0}
    return {'edge_novelty': new / E, 'edge_density': E / (U * (U - 1)) if U >= 2 else 0.0, 'new_edge_count': new}


@hook
class NodeAnalyticsHook(StatefulHook):
    """Compute node-centric statistics for a specific set of tracked nodes, with state across batches.

    Args:
        tracked_nodes (Tensor): 1D tensor of node IDs to track statistics for.
        num_nodes (int): Total number of nodes in the graph.
        id (str): A unique identifier for the hook. The hook's name and all attributes it produces are suffixed with it.
        capacity (int): (extension) initial slots of each device table, rounded up to a power of two.

    Produces ``node_stats`` (node id -> degree, activity, new_neighbors, lifetime, time_since_last_seen, appearances), ``node_macro_stats``
    (node_novelty, new_node_count) and ``edge_stats`` (edge_novelty, edge_density, new_edge_count).

    Key words: node-level statistics.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time', 'node_x_time', 'node_x_nids'}
    _cls_produces = {'node_stats', 'node_macro_stats', 'edge_stats'}

    def __init__(self, tracked_nodes: Tensor, num_nodes: int, id: Optional[str] = None, capacity: Optional[int] = None) -> None:
        super().__init__()
        if num_nodes <= 0:
            raise ValueError('num_nodes must be positive')
        self.tracked_nodes = tracked_nodes.unique()
        self.num_nodes = num_nodes
        self._tracked_mask = torch.zeros(num_nodes, dtype=torch.bool)
        self._tracked_mask[self.tracked_nodes.long().cpu()] = True
        self._tracked_list: List[int] = [int(n) for n in self.tracked_nodes.tolist()]
        self._tracked_set = set(self._tracked_list)
        cap = _DEFAULT_CAPACITY if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError('capacity must be positive')
        self._capacity0 = 1 << (cap - 1).bit_length()
        self._dev: Optional[dict] = None
        self._calls = 0  # device calls over the hook's life (the per-node stamps compare against it): never reset
        self._status = 0
        self.rehashes = 0  # table growths on the device (tests, tools)
        self._id = id
        self._clear_host()
        self.__post_init__()

    def _clear_host(self) -> None:
        self._first_seen: Dict[int, Any] = {}
        self._last_seen: Dict[int, Any] = {}
        self._appearances: Dict[int, int] = {}
        self._total_timesteps: Set[Any] = set()
        self._node_timesteps: Dict[int, Set[Any]] = {n: set() for n in self._tracked_list}
        self._all_neighbors: Dict[int, Set[int]] = {n: set() for n in self._tracked_list}
        self._seen_edges: Set[Tuple[int, int]] = set()

    def reset_state(self) -> None:
        """Reset internal state (on the device: fills in place, nothing read back)."""
        self._clear_host()
        d = self._dev
        if d is not None:
            for k in _TABLES:
                d[k].fill_(-1)
            for k in ('first', 'last'):
                d[k].fill_(-1)
            for k in ('appearances', 'counters', 'degree', 'new_nbrs', 'present', 'scalars'):
                d[k].zero_()
            d['occ'] = dict.fromkeys(_TABLES, 0)

    def check(self) -> None:
        """Raise ``ValueError`` (once) for what the kernels flagged since the last check: an id outside ``[0, num_nodes)``, a negative time
        (or more than 2^32 distinct ones), or a table that ran full (the capacity rule makes that a bug).  One device-to-host read."""
        if self._dev is not None:
            bits = int(self._dev['counters'][4])
            if bits:
                self._dev['counters'][4:5].zero_()
            self._status |= bits
        bits, self._status = self._status, 0
        if bits & _native.AN_BAD_ID:
            raise ValueError(f'NodeAnalyticsHook: ids must lie in [0, {self.num_nodes}); an event with an id outside was offered (it took no part)')
        if bits & _native.AN_BAD_TIME:
            raise ValueError('NodeAnalyticsHook: the device path takes integer times >= 0 and fewer than 2^32 distinct ones (an event outside took no part)')
        if bits & _native.AN_TABLE_FULL:
            raise ValueError('NodeAnalyticsHook: a device table ran full (entries were dropped)')

    def state(self) -> Dict[str, Any]:
        """The state as plain Python data, the same from either path (for tests and debugging; on the device it reads everything back):
        first / last / appearances by tracked node seen so far, and the key sets edges {(src, dst)}, nbrs {(node, neighbour)}, times {t},
        apps {(node, t)}."""
        if self._dev is None:
            return dict(first=dict(self._first_seen), last=dict(self._last_seen), appearances=dict(self._appearances), edges=set(self._seen_edges),
                        nbrs={(n, m) for n, s in self._all_neighbors.items() for m in s}, times=set(self._total_timesteps),
                        apps={(n, t) for n, s in self._node_timesteps.items() for t in s})  # fmt: skip
        d = self._dev
        first, last, app = (d[k].tolist() for k in ('first', 'last', 'appearances'))
        seen = [i for i, v in enumerate(last) if v >= 0]
        rows = {k: [r for r in d[k].tolist() if r[0] != -1] for k in _TABLES}
        node = self._tracked_list
        time_of = {tid: t for t, tid in rows['times']}
        return dict(first={node[i]: first[i] for i in seen}, last={node[i]: last[i] for i in seen}, appearances={node[i]: app[i] for i in seen},
                    edges={(k >> 32, k & 0xFFFFFFFF) for k, _ in rows['edges']}, nbrs={(node[k >> 32], k & 0xFFFFFFFF) for k, _ in rows['nbrs']},
                    times=set(time_of.values()), apps={(node[k >> 32], time_of[k & 0xFFFFFFFF]) for k, _ in rows['apps']})  # fmt: skip

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        fields = (batch.edge_src, batch.edge_dst, batch.edge_time, getattr(batch, 'node_x_nids', None), getattr(batch, 'node_x_time', None))
        device = next((t.device for t in fields if t is not None), torch.device('cpu'))
        step = self._step_device if device.type == 'cuda' else self._step_host
        node_stats, macro, edge = step(fields, device)
        if fields[0] is None and fields[1] is None and fields[3] is None:  # no ids at all: written without the id suffix, as the reference does
            batch.node_stats, batch.node_macro_stats, batch.edge_stats = {}, macro, edge  # type: ignore[attr-defined]
            return batch
        self.add_batch_attribute(batch, 'node_stats', node_stats)
        self.add_batch_attribute(batch, 'node_macro_stats', macro)
        self.add_batch_attribute(batch, 'edge_stats', edge)
        return batch

    # ---- host tensors ------------------------------------------------------------------------------------------------------------------

    def _step_host(self, fields, device):
        src, dst, et, nids, nt = (None if t is None else t.reshape(-1).tolist() for t in fields)
        latest_edge = max(et) if et else 0.0
        latest_node = max(nt) if nt else 0.0
        current = max(latest_edge, latest_node)
        for times in (et, nt):
            if times:
                self._total_timesteps.update(times)
        id_fields = [f for f in (src, dst, nids) if f is not None]
        if not id_fields:
            return {}, _node_macro(0, 0), _edge_stats(0, 0, 0)
        batch_nodes = sorted(set().union(*id_fields))
        if batch_nodes and not (0 <= batch_nodes[0] and batch_nodes[-1] < self.num_nodes):
            bad = batch_nodes[0] if batch_nodes[0] < 0 else batch_nodes[-1]
            raise IndexError(f'index {bad} is out of bounds for dimension 0 with size {self.num_nodes}')
        present = [n for n in batch_nodes if n in self._tracked_set]
        degree = dict.fromkeys(present, 0)
        nbrs: Dict[int, Set[int]] = {n: set() for n in present}
        times_of: Dict[int, Set[Any]] = {n: set() for n in present}
        if src is not None and dst is not None:
            for s, d in zip(src, dst):
                if s in degree:
                    nbrs[s].add(d)
                if d in degree:
                    nbrs[d].add(s)
            for n in src + dst:
                if n in degree:
                    degree[n] += 1
        for ids, times in ((src, et), (dst, et), (nids, nt)):
            if ids is not None and times is not None:
                for n, t in zip(ids, times):
                    if n in times_of:
                        times_of[n].add(t)
        node_stats: Dict[int, Dict[str, Any]] = {}
        total = len(self._total_timesteps) or 1
        for n in present:
            self._first_seen.setdefault(n, current)
            self._last_seen[n] = current
            self._node_timesteps[n] |= times_of[n]
            self._appearances[n] = len(self._node_timesteps[n])
            new = nbrs[n] - self._all_neighbors[n]
            self._all_neighbors[n] |= nbrs[n]
            node_stats[n] = {'degree': degree[n], 'activity': self._appearances[n] / total, 'new_neighbors': len(new),
                             'lifetime': current - self._first_seen[n], 'time_since_last_seen': 0.0, 'appearances': self._appearances[n]}  # fmt: skip
        for n in self._tracked_list:
            if n not in node_stats and n in self._last_seen:
                node_stats[n] = {'degree': 0, 'activity': self._appearances.get(n, 0) / total, 'new_neighbors': 0,
                                 'lifetime': self._last_seen[n] - self._first_seen[n], 'time_since_last_seen': current - self._last_seen[n],
                                 'appearances': self._appearances.get(n, 0)}  # fmt: skip
        untracked = sum(1 for n in nids if n not in self._tracked_set) if nids else 0
        new_edges, E, U = 0, 0, 0
        if src is not None and dst is not None and src:
            E = len(src)
            for pair in zip(src, dst):
                if pair not in self._seen_edges:
                    new_edges += 1
                    self._seen_edges.add(pair)
            U = len(set(src) | set(dst))
        return node_stats, _node_macro(untracked, len(nids) if nids else 0), _edge_stats(new_edges, E, U)

    # ---- device tensors ----------------------------------------------------------------------------------------------------------------

    def _device_state(self, device: torch.device) -> dict:
        d = self._dev
        if d is None or d['device'] != device:
            T = len(self._tracked_list)
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)
            slot_of = torch.full((self.num_nodes,), -1, dtype=torch.int32)
            slot_of[self.tracked_nodes.long().cpu()] = torch.arange(T, dtype=torch.int32)
            d = self._dev = dict(device=device, slot_of=slot_of.to(device), first=torch.full((T,), -1, dtype=torch.int64, device=device),
                                 last=torch.full((T,), -1, dtype=torch.int64, device=device), appearances=z(T, torch.int64), counters=z(8, torch.int64),
                                 degree=z(T, torch.int32), new_nbrs=z(T, torch.int32), present=z(T, torch.int32), stamp=z(self.num_nodes, torch.int32),
                                 scalars=z(16, torch.int64), occ=dict.fromkeys(_TABLES, 0))  # fmt: skip
            for k in _TABLES:
                d[k] = torch.full((self._capacity0, 2), -1, dtype=torch.int64, device=device)
        return d

    def _grow(self, d: dict, incoming: Dict[str, int], device: torch.device) -> None:
        from ...nn.edgebank import grow_capacity

        lib = None
        for k in _TABLES:
            cap = d[k].shape[0]
            need = grow_capacity(cap, 0, d['occ'][k], incoming[k])
            if need == cap:
                continue
            lib = lib or _native.load()
            grown = torch.full((need, 2), -1, dtype=torch.int64, device=device)
            rc = lib.tgmx_node_analytics_rehash(d[k].data_ptr(), cap, grown.data_ptr(), need, d['counters'][4:].data_ptr(), _native.stream_ptr(device.index))
            if rc:
                _native.check(rc, 'tgmx_node_analytics_rehash')
            d[k] = grown
            self.rehashes += 1

    def _step_device(self, fields, device):
        if (fields[0] is None) != (fields[1] is None):
            raise ValueError('NodeAnalyticsHook on the device needs edge_src and edge_dst together')
        names = ('edge_src', 'edge_dst', 'edge_time', 'node_x_nids', 'node_x_time')
        require_on(device, 'NodeAnalyticsHook', **dict(zip(names, fields)))
        src, dst, et, nids, nt = (_native_vector(t, n) for t, n in zip(fields, names))
        b = an_batch(src, dst, et, nids, nt)
        if (b.E and src.numel() != dst.numel()) or (et is not None and src is not None and b.Et != b.E) or (nt is not None and nids is not None and b.Nt != b.Nn):
            raise ValueError(f'NodeAnalyticsHook: field lengths differ (edges {b.E}, edge times {b.Et}, node events {b.Nn}, node times {b.Nt})')
        d = self._device_state(device)
        # the batch's worst case: every edge a new pair, both ends tracked and new neighbours, every time new, every (node, time) new
        self._grow(d, dict(edges=b.E, nbrs=2 * b.E, times=b.Et + b.Nt, apps=2 * b.E + b.Nn), device)
        T = len(self._tracked_list)
        st = _native.NodeAnalytics(d['slot_of'].data_ptr(), self.num_nodes, T, d['first'].data_ptr(), d['last'].data_ptr(), d['appearances'].data_ptr(),
                                   d['edges'].data_ptr(), d['edges'].shape[0], d['nbrs'].data_ptr(), d['nbrs'].shape[0], d['times'].data_ptr(),
                                   d['times'].shape[0], d['apps'].data_ptr(), d['apps'].shape[0], d['counters'].data_ptr(), d['degree'].data_ptr(),
                                   d['new_nbrs'].data_ptr(), d['present'].data_ptr(), d['stamp'].data_ptr(), d['scalars'].data_ptr())  # fmt: skip
        self._calls += 1
        out = torch.empty((T + 2, 8), dtype=torch.int64, device=device)
        rc = _native.load().tgmx_node_analytics_step(ctypes.byref(st), ctypes.byref(b), self._calls, out.data_ptr(), _native.stream_ptr(device.index))
        if rc:
            _native.check(rc, 'tgmx_node_analytics_step')
        rows = out.tolist()  # the one read of the batch
        num_times, new_edges, U, E, Nn, untracked, current, bits = rows[T]
        d['occ'] = dict(zip(_TABLES, rows[T + 1][:4]))
        if bits:
            d['counters'][4:5].zero_()
            self._status |= bits
        total = num_times or 1
        node_stats: Dict[int, Dict[str, Any]] = {}
        node = self._tracked_list
        for flag in (2, 1):  # the nodes present (ascending id), then the absent ones seen before (tracked order): both are index order
            for i in range(T):
                r = rows[i]
                if r[0] == flag:
                    node_stats[node[i]] = {'degree': r[1], 'activity': r[2] / total, 'new_neighbors': r[3], 'lifetime': r[4],
                                           'time_since_last_seen': 0.0 if flag == 2 else r[5], 'appearances': r[2]}  # fmt: skip
        if src is None and nids is None:
            return {}, _node_macro(0, 0), _edge_stats(0, 0, 0)
        return node_stats, _node_macro(untracked, Nn), _edge_stats(new_edges, E, U)
