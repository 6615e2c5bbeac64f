"""tCoMemPredictor (the reference's ``tgm/nn/modules/t_comem.py``) with its state on the device.

The reference updates in a Python loop over ``.tolist()``-ed events and ends every query in a Python loop with two ``.item()`` calls per
pair; three of its state tensors are created without a device, so it cannot hold its state on a GPU at all.  Here the per-node rings, the
popularity counts and the pair counts live on the device (``csrc/tcomem.hip``): ``update`` is one launch per 1024 events, a query call is one
launch whatever its size, and ``query_one_vs_many`` answers a whole evaluation batch (every positive edge with its own negatives) in one
launch, one wave per positive.  ``update`` and the queries read nothing back from the device; the window properties, the inspection views,
``check()`` and a growth of the pair table do.

Reference behaviours that are kept, on purpose (the g20 fixtures pin each of them):

* ``window_ratio`` is validated and never used: the window size is ``clamp(max(ts) - min(ts), min=1.0)`` of the constructor's events, once;
* the window arithmetic is float32: ``start = f32(f32(end) - size)``; with Unix-scale timestamps every quantity is a multiple of 128;
* every event enters its source's ring, whatever its timestamp, and the stored timestamp is rounded to float32;
* both directions of a pair are counted, so a self-loop counts 2;
* the co-occurrence term is stored into ``zeros_like(query_src)``: with integer queries (what the Base3 example passes) it is truncated to
  0 for every pair and the answer is the base score alone; float32 queries add it rounded to float32, float64 queries add it in double and
  round the sum.  The answer is float32 always.  ``co_occurrence_on_integer_queries=True`` is NOT the reference: integer queries then take
  the float32 rule.

Ids lie in ``[0, 2^31)``, sources and an update's destinations below ``num_nodes`` (the reference raises ``IndexError`` for those; here the
event or query is ignored, answers 0 and sets a bit that :meth:`tCoMemPredictor.check` raises ``ValueError`` for).  Ids and timestamps are
int32 / int64 (read in place) or floating tensors of integral values (taken through ``.long()``).  Non-integral timestamps, ``|ts| >= 2^53``
and popularity counts at or above 2^24 are not supported.
"""
from __future__ import annotations

from types import MappingProxyType
from typing import List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from .. import _native
from ..core.neg_batch_list import uniform_matrix
from ._fwd_plumbing import ids as _ids, pow2ceil as _pow2ceil
from .edgebank import EdgeBankPredictor, grow_capacity

_EMPTY = -1  # the empty key, all ones, as the int64 the table tensor shows
_QUERY_DTYPES = {torch.int32: 0, torch.int64: 1, torch.float32: 2, torch.float64: 3}
_STATE_WORDS = 2  # tgmx_tcomem_state_bytes() / 8
STATUS_BAD_ID, STATUS_OVERFLOW, STATUS_BAD_SRC, STATUS_BAD_DST = 1, 2, 4, 8


class tCoMemPredictor:
    def __init__(
        self,
        src: torch.Tensor,
        dst: torch.Tensor,
        ts: torch.Tensor,
        num_nodes: int,
        k: int = 50,
        window_ratio: float = 0.15,
        co_occurrence_weight: float = 0.8,
        *,
        capacity: Optional[int] = None,
        co_occurrence_on_integer_queries: bool = False,
    ) -> None:
        """The t-CoMem baseline (https://www.arxiv.org/abs/2506.12764): recent-neighbour popularity inside a time window plus pair counts.

        Args:
            src, dst, ts: the edges the memory starts with.
            num_nodes: number of nodes; sources and update destinations lie below it.
            k: length of each node's ring of recent events, ``0 < k <= num_nodes``.
            window_ratio: validated to lie in ``(0, 1]`` and otherwise unused, as in the reference.
            co_occurrence_weight: weight of the pair-count term, in ``(0, 1]``.
            capacity: initial number of slots of the pair table (rounded up to a power of two; the table grows by itself).
            co_occurrence_on_integer_queries: not the reference.  When set, int32 / int64 queries add the co-occurrence term as float32
                queries do, instead of the reference's truncation of it to 0.
        """
        if not 0 < window_ratio <= 1.0:
            raise ValueError('Window ratio must be in (0, 1]')
        if not 0 < co_occurrence_weight <= 1.0:
            raise ValueError('Co-occurrence weight must be in (0, 1]')
        if 0 >= k:
            raise ValueError('K must be positive')
        if num_nodes <= 0:
            raise ValueError('``num_nodes`` must be set to the total number of nodes.')
        if k > num_nodes:
            raise ValueError('``k`` must be smaller than ``num_nodes``.')
        self._check_input_data(src, dst, ts)
        for name, t in (('src', src), ('dst', dst), ('ts', ts)):
            _native.require_device(t, f'tCoMemPredictor: {name}')
        if num_nodes > 1 << 31:
            raise ValueError('tCoMemPredictor: num_nodes must not exceed 2^31')
        self._lib = _native.load()

        self._window_ratio = window_ratio
        self.device = self._device = src.device
        self.num_nodes, self.k = int(num_nodes), int(k)
        self.co_occurrence_weight = co_occurrence_weight
        self.co_occurrence_on_integer_queries = bool(co_occurrence_on_integer_queries)

        N, K = self.num_nodes, self.k
        ring = torch.empty(N, K, 2, dtype=torch.int32, device=self._device)  # {float32 ts, int32 dst}
        ring[..., 0].view(torch.float32).fill_(-float('inf'))
        ring[..., 1] = -1
        self._ring = ring
        self._node = torch.zeros(3, N, dtype=torch.int32, device=self._device)  # pos, len, popularity
        self._status = torch.zeros(1, dtype=torch.int32, device=self._device)
        self._kept_dev = torch.zeros(1, dtype=torch.int64, device=self._device)
        n = len(src)
        self._capacity = max(_pow2ceil(capacity) if capacity else 0, grow_capacity(0, 0, 0, n))
        self._alloc(self._capacity)
        # the reference's own expressions, on the device: end = max(ts), size = clamp(max(ts) - min(ts), min=1.0), float32
        t = _ids(ts)
        self._state[0] = t.max().long()
        self._state[1:2].view(torch.float32)[0] = torch.clamp(t.max().long() - t.min().long(), min=1.0)
        self._offered = 0  # events offered since the last rehash
        self._kept = 0  # pairs the last rehash kept
        self.rehashes = 0

        self.update(src, dst, ts)

    # ---- the pair table -------------------------------------------------------------------------------------------------------------------
    def _alloc(self, capacity: int) -> None:
        # one buffer: the slots, then the state block behind them
        buf = torch.empty(2 * capacity + _STATE_WORDS, dtype=torch.int64, device=self._device)
        slots = buf[: 2 * capacity].view(capacity, 2)
        slots[:, 0] = _EMPTY
        slots[:, 1] = 0
        buf[2 * capacity :] = 0
        self._buf, self._state = buf, buf[2 * capacity :]

    def _block(self) -> _native.TCoMem:
        node = self._node
        return _native.TCoMem(self._ring.data_ptr(), node[0].data_ptr(), node[1].data_ptr(), node[2].data_ptr(), self._buf.data_ptr(), self._capacity,
                              self._state.data_ptr(), self.num_nodes, self.k, 0, float(self.co_occurrence_weight), self._status.data_ptr())  # fmt: skip

    def _stream(self) -> int:
        return _native.stream_ptr(self._device.index)

    def _reserve(self, incoming: int) -> None:
        capacity = grow_capacity(self._capacity, self._offered, self._kept, incoming)
        if capacity == self._capacity:
            return
        old = self._block()
        keep = self._buf  # alive until the launch is enqueued
        state = self._state
        self._capacity = capacity
        self._alloc(capacity)
        self._state.copy_(state)
        _native.check(self._lib.tgmx_tcomem_rehash(old, self._block(), self._kept_dev.data_ptr(), self._stream()), 'tgmx_tcomem_rehash')
        del keep
        self._kept = int(self._kept_dev.item())  # the one read a rehash does
        self._offered = 0
        self.rehashes += 1

    @property
    def capacity(self) -> int:
        return self._capacity

    # ---- the reference's surface ----------------------------------------------------------------------------------------------------------
    def update(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor) -> None:
        """One batch of edges into the memory, one launch per 1024 edges; the argument checks are the constructor's."""
        self._check_input_data(src, dst, ts)
        for name, t in (('src', src), ('dst', dst), ('ts', ts)):
            _native.require_device(t, f'tCoMemPredictor.update: {name}')
        n = len(src)
        self._reserve(n)
        s, d, t = _ids(src), _ids(dst), _ids(ts)
        _native.check(
            self._lib.tgmx_tcomem_update(self._block(), s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64, t.data_ptr(),
                                         t.dtype == torch.int64, n, self._stream()),
            'tgmx_tcomem_update',
        )  # fmt: skip
        self._offered += n

    def _code(self, dtype: torch.dtype) -> int:
        if dtype not in _QUERY_DTYPES:
            raise TypeError(f'tCoMemPredictor takes int32, int64, float32 or float64 queries, got {dtype}')
        code = _QUERY_DTYPES[dtype]
        return 2 if code < 2 and self.co_occurrence_on_integer_queries else code

    def __call__(self, query_src: torch.Tensor, query_dst: torch.Tensor) -> torch.Tensor:
        """One launch for the whole call: float32 scores, the base score of the source plus the co-occurrence term as the dtype of
        ``query_src`` makes the reference add it (see the module's notes)."""
        _native.require_device(query_src, 'tCoMemPredictor: query_src')
        _native.require_device(query_dst, 'tCoMemPredictor: query_dst')
        code = self._code(query_src.dtype)
        n = query_src.numel()
        pred = torch.zeros(query_src.shape, dtype=torch.float32, device=query_src.device)
        if n == 0:
            return pred
        if query_dst.numel() < n:  # the reference's zip() stops at the shorter one
            raise ValueError(f'query_dst has {query_dst.numel()} entries for {n} sources')
        s, d = _ids(query_src), _ids(query_dst)
        _native.check(
            self._lib.tgmx_tcomem_query(self._block(), s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64, None, 0, None, 0,
                                        n, n, pred.data_ptr(), code, self._stream()),
            'tgmx_tcomem_query',
        )  # fmt: skip
        return pred

    def query_one_vs_many(
        self, src: torch.Tensor, dst: torch.Tensor, negatives: Union[torch.Tensor, Sequence[torch.Tensor]]
    ) -> Union[torch.Tensor, List[torch.Tensor]]:
        """The evaluation loop's ``B`` calls as one launch: row ``b`` answers ``(src[b], dst[b])`` in column 0 and ``(src[b], negatives[b][m])``
        after it, with the bits ``self(src[b].repeat(1 + M), cat([dst[b:b+1], negatives[b]]))`` gives.  ``negatives`` is ``[B, M]`` (the
        result is ``[B, 1 + M]``) or a list of ``B`` 1-D tensors of any lengths, ``batch.neg_batch_list`` (the result is a list of ``B``
        tensors).  The answers are float32; ``src``'s dtype decides the co-occurrence term."""
        _native.require_device(src, 'tCoMemPredictor.query_one_vs_many: src')
        _native.require_device(dst, 'tCoMemPredictor.query_one_vs_many: dst')
        code = self._code(src.dtype)
        B = src.numel()
        if dst.numel() != B:
            raise ValueError(f'mismatch shape: src: {B}, dst: {dst.numel()}')
        as_rows = uniform_matrix(negatives)  # a NegBatchList of equal rows: its matrix, no B-way cat
        if as_rows is not None:
            negatives = as_rows
        ragged = not isinstance(negatives, torch.Tensor)
        if ragged:
            negatives = list(negatives)
            if len(negatives) != B:
                raise ValueError(f'negatives holds {len(negatives)} rows for {B} positive edges')
            sizes = [int(t.numel()) for t in negatives]
            for t in negatives:
                _native.require_device(t, 'tCoMemPredictor.query_one_vs_many: negatives')
            if B == 0:
                return []
            neg = _ids(torch.cat([t.reshape(-1) for t in negatives]))
            off_host = np.zeros(B + 1, dtype=np.int64)
            np.cumsum(sizes, out=off_host[1:])
            # host to device, from pinned memory so that the host does not wait: the sizes are shapes, nothing is read back
            off = torch.from_numpy(off_host).pin_memory().to(self._device, non_blocking=True)
            M, total = 0, B + int(off_host[-1])
        else:
            _native.require_device(negatives, 'tCoMemPredictor.query_one_vs_many: negatives')
            if negatives.dim() != 2 or negatives.shape[0] != B:
                raise ValueError(f'negatives must be [B, M] with B = {B}, got {tuple(negatives.shape)}')
            neg, off = _ids(negatives), None
            M = int(negatives.shape[1])
            total = B * (M + 1)
        pred = torch.zeros(total, dtype=torch.float32, device=src.device)
        if total:
            s, d = _ids(src), _ids(dst)
            _native.check(
                self._lib.tgmx_tcomem_query(self._block(), s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64,
                                            neg.data_ptr() if neg.numel() else d.data_ptr(), neg.dtype == torch.int64, _native.ptr(off), M, B, total,
                                            pred.data_ptr(), code, self._stream()),
                'tgmx_tcomem_query',
            )  # fmt: skip
        if not ragged:
            return pred.view(B, M + 1) if as_rows is None else list(pred.view(B, M + 1).unbind(0))
        return list(torch.split(pred, [m + 1 for m in sizes]))

    # ---- reads from the device ------------------------------------------------------------------------------------------------------------
    def _window(self):
        """(end, float32 end, float32 size, float32 start) from the state block, the start as every query recomputes it"""
        w = self._state.cpu().numpy()
        end, size = int(w[0]), w[1:2].view(np.float32)[0]
        endf = np.float32(end)
        return end, endf, size, np.float32(endf - size)

    @property
    def window_start(self) -> float:
        """Where the window starts now (one read from the device): ``f32(f32(window_end) - size)``."""
        return float(self._window()[3])

    @property
    def window_end(self) -> int:
        """The largest timestamp offered so far (one read from the device)."""
        return self._window()[0]

    @property
    def window_ratio(self) -> float:
        """The ``window_ratio`` the predictor was built with (the reference never uses it)."""
        return self._window_ratio

    @property
    def window_size(self) -> int:
        """``int(window_end - window_start)`` in the reference's float32 arithmetic (one read from the device)."""
        _, endf, _, start = self._window()
        return int(np.float32(endf - start))

    @property
    def recent_ts(self) -> torch.Tensor:
        """``[num_nodes, k]`` float32 on the host, -inf where empty (a copy, for inspection)."""
        return self._ring[..., 0].cpu().contiguous().view(torch.float32)

    @property
    def recent_dst(self) -> torch.Tensor:
        """``[num_nodes, k]`` int64 on the host, -1 where empty (a copy, for inspection)."""
        return self._ring[..., 1].cpu().long()

    @property
    def recent_pos(self) -> torch.Tensor:
        return self._node[0].cpu().float()

    @property
    def recent_len(self) -> torch.Tensor:
        return self._node[1].cpu().float()

    @property
    def popularity(self) -> torch.Tensor:
        """``[num_nodes]`` float32 on the host: how often each node was a destination."""
        return self._node[2].cpu().float()

    @property
    def node_to_co_occurrence(self) -> Mapping[int, Mapping[int, int]]:
        """``{a: {b: count}}`` with both directions, as the reference's nested dict holds it, built from the pair table by one
        device-to-host copy (read-only, sorted by id; for inspection, not for the loop)."""
        slots = self._buf[: 2 * self._capacity].cpu().numpy().reshape(self._capacity, 2)
        live = slots[:, 0] != _EMPTY
        key, count = slots[live, 0], slots[live, 1]
        lo, hi = key >> 32, key & 0xFFFFFFFF
        a, b, c = np.concatenate([lo, hi[lo != hi]]), np.concatenate([hi, lo[lo != hi]]), np.concatenate([count, count[lo != hi]])
        order = np.lexsort((b, a))
        nested: dict = {}
        for x, y, z in zip(a[order].tolist(), b[order].tolist(), c[order].tolist()):
            nested.setdefault(x, {})[y] = z
        return MappingProxyType({x: MappingProxyType(row) for x, row in nested.items()})

    def check(self) -> None:
        """Raise ``ValueError`` for what the kernels flagged since the last check (one device-to-host read): an id outside ``[0, 2^31)``,
        a source or an update's destination at or above ``num_nodes``, or a pair table that ran full."""
        bits = int(self._status.item())
        if bits:
            self._status.zero_()
        if bits & STATUS_BAD_ID:
            raise ValueError('tCoMemPredictor: node ids must lie in [0, 2^31); an id outside was offered or queried (it was ignored)')
        if bits & STATUS_BAD_SRC:
            raise ValueError('tCoMemPredictor: a source at or above num_nodes was offered or queried (it was ignored)')
        if bits & STATUS_BAD_DST:
            raise ValueError('tCoMemPredictor: an update held a destination at or above num_nodes (the event was ignored)')
        if bits & STATUS_OVERFLOW:
            raise ValueError('tCoMemPredictor: a probe ran through the whole pair table (events were dropped)')

    _check_input_data = staticmethod(EdgeBankPredictor._check_input_data)
