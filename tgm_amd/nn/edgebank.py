"""EdgeBankPredictor (the reference's ``tgm/nn/modules/edgebank.py``) with its memory as a hash table on the device.

The reference keeps a Python ``dict`` and walks it one ``.tolist()``-ed query at a time.  Here the dict is an open-addressing table of
16-byte slots (``csrc/edgebank.hip``): ``update`` is one launch per loader batch, a query call is one launch whatever its size, and
``query_one_vs_many`` answers a whole evaluation batch (every positive edge with its own negatives) in one launch.  ``update`` and the
queries read nothing back from the device; ``window_start``, ``window_end``, ``memory``, ``check()`` and a growth of the table do.

Reference behaviours that are kept, on purpose (the g19 fixtures pin each of them):

* in ``'fixed'`` mode the window arithmetic is float32, as the reference's 0-dim tensors make it: with Unix-scale timestamps the window
  size and start are multiples of 128;
* an event is stored only if ``ts >= window_start`` (after the batch has moved the window), in BOTH modes: ``'unlimited'`` drops an event
  older than the start of the current window;
* the stored timestamp is that of the last arrival which passed that test, not the largest;
* the result is ``zeros_like(query_src)`` with ``pos_prob`` written into it: integer queries with ``pos_prob=0.7`` answer all zeros.

Ids lie in ``[0, 2^31)``; ids and timestamps are int32 / int64 (read in place) or floating tensors of integral values (taken through
``.long()``).  Non-integral timestamps and ``|ts| >= 2^53`` are not supported.  An id outside the range contributes nothing and answers 0;
it sets a bit in a status word on the device, and :meth:`EdgeBankPredictor.check` raises ``ValueError`` for it.
"""
from __future__ import annotations

from types import MappingProxyType
from typing import Any, List, Literal, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _native
from ..core.neg_batch_list import uniform_matrix
from ._fwd_plumbing import ids as _ids, pow2ceil as _pow2ceil

_EMPTY = -1  # the empty key, all ones, as the int64 the table tensor shows
_OUT_DTYPES = {torch.int32: 0, torch.int64: 1, torch.float32: 2, torch.float64: 3}
_STATE_WORDS = 4  # tgmx_edgebank_state_bytes() / 8
STATUS_BAD_ID, STATUS_OVERFLOW = 1, 2


def grow_capacity(capacity: int, offered: int, kept: int, incoming: int) -> int:
    """The capacity the table needs before ``incoming`` more events are offered: at least twice (the events offered since the last rehash +
    the entries that rehash kept + the incoming ones), a power of two, never smaller than it is.  Every event may be a new pair, and the
    host counts events, not pairs: the load never passes 0.5 without a read from the device."""
    need = 2 * (offered + kept + incoming)
    return capacity if need <= capacity else _pow2ceil(need)


class EdgeBankPredictor:
    def __init__(
        self,
        src: torch.Tensor,
        dst: torch.Tensor,
        ts: torch.Tensor,
        memory_mode: Literal['unlimited', 'fixed'] = 'unlimited',
        window_ratio: float = 0.15,
        pos_prob: float = 1.0,
        *,
        capacity: Optional[int] = None,
    ) -> None:
        """The EdgeBank baseline (https://arxiv.org/abs/2207.10128): an edge is predicted iff it was seen before (and recently, in fixed mode).

        Args:
            src, dst, ts: the edges the memory starts with.
            memory_mode: ``'unlimited'`` keeps every observed edge, ``'fixed'`` only those inside a sliding time window.
            window_ratio: length of the window over the time span of the initial edges, in ``(0, 1]`` (``'fixed'`` only).
            pos_prob: what an edge found in memory answers.
            capacity: initial number of slots (rounded up to a power of two; the table grows by itself).
        """
        if memory_mode != 'unlimited' and memory_mode != 'fixed':
            raise ValueError('memory_mode must be "unlimited" or "fixed"')
        if window_ratio <= 0 or window_ratio > 1.0:
            raise ValueError('Window ratio must be in (0, 1]')
        self._check_input_data(src, dst, ts)
        for name, t in (('src', src), ('dst', dst), ('ts', ts)):
            _native.require_device(t, f'EdgeBankPredictor: {name}')
        self._lib = _native.load()

        self.pos_prob = pos_prob
        self._window_ratio = window_ratio
        self._fixed_memory = memory_mode == 'fixed'
        self._device = src.device

        # the reference's own expressions, on the device: in fixed mode the Python float makes the start, and so the size, float32
        t = _ids(ts)
        window_start, window_end = t.min().long(), t.max().long()
        if self._fixed_memory:
            window_start = t.max().long() - window_ratio * (t.max().long() - t.min().long())
        window_size = window_end - window_start

        n = len(src)
        self._capacity = max(_pow2ceil(capacity) if capacity else 0, grow_capacity(0, 0, 0, n))
        self._alloc(self._capacity)
        self._state[0] = window_end
        if self._fixed_memory:
            self._state[2:3].view(torch.float32)[0] = window_size
        else:
            self._state[1] = window_size
        self._status = torch.zeros(1, dtype=torch.int32, device=self._device)
        self._kept_dev = torch.zeros(1, dtype=torch.int64, device=self._device)
        self._arrivals = 0  # events offered so far (the next event's arrival number - 1)
        self._offered = 0  # events offered since the last rehash
        self._kept = 0  # entries the last rehash kept
        self.rehashes = 0

        self.update(src, dst, ts)

    # ---- the table ------------------------------------------------------------------------------------------------------------------------
    def _alloc(self, capacity: int) -> None:
        # one buffer: the slots, then the state block behind them, so that `memory` is one device-to-host copy
        buf = torch.empty(2 * capacity + _STATE_WORDS, dtype=torch.int64, device=self._device)
        slots = buf[: 2 * capacity].view(capacity, 2)
        slots[:, 0] = _EMPTY
        slots[:, 1] = 0
        buf[2 * capacity :] = 0
        self._buf, self._state = buf, buf[2 * capacity :]
        self._stamp = torch.zeros(capacity, dtype=torch.int64, device=self._device)

    def _block(self) -> _native.EdgeBank:
        return _native.EdgeBank(self._buf.data_ptr(), self._stamp.data_ptr(), self._capacity, self._state.data_ptr(), int(self._fixed_memory), 0,
                                float(self.pos_prob), self._arrivals, self._status.data_ptr())  # fmt: skip

    def _stream(self) -> int:
        return _native.stream_ptr(self._device.index)

    def _reserve(self, incoming: int) -> None:
        capacity = grow_capacity(self._capacity, self._offered, self._kept, incoming)
        if capacity == self._capacity:
            return
        old = self._block()
        keep = (self._buf, self._stamp)  # alive until the launch is enqueued
        state = self._state
        self._capacity = capacity
        self._alloc(capacity)
        self._state.copy_(state)
        _native.check(self._lib.tgmx_edgebank_rehash(old, self._block(), self._kept_dev.data_ptr(), self._stream()), 'tgmx_edgebank_rehash')
        del keep
        self._kept = int(self._kept_dev.item())  # the one read a rehash does
        self._offered = 0
        self.rehashes += 1

    @property
    def capacity(self) -> int:
        return self._capacity

    # ---- the reference's surface ----------------------------------------------------------------------------------------------------------
    def update(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor) -> None:
        """One batch of edges into the memory, in one launch (three for more than 1024 edges); the argument checks are the constructor's."""
        self._check_input_data(src, dst, ts)
        for name, t in (('src', src), ('dst', dst), ('ts', ts)):
            _native.require_device(t, f'EdgeBankPredictor.update: {name}')
        n = len(src)
        self._reserve(n)
        s, d, t = _ids(src), _ids(dst), _ids(ts)
        _native.check(
            self._lib.tgmx_edgebank_update(self._block(), s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64, t.data_ptr(),
                                           t.dtype == torch.int64, n, self._stream()),
            'tgmx_edgebank_update',
        )  # fmt: skip
        self._arrivals += n
        self._offered += n

    def __call__(self, query_src: torch.Tensor, query_dst: torch.Tensor) -> torch.Tensor:
        """One launch for the whole call: ``zeros_like(query_src)`` with ``pos_prob`` (cast to that dtype) where the
        edge is in memory and, in fixed mode, its stored timestamp is inside the window."""
        _native.require_device(query_src, 'EdgeBankPredictor: query_src')
        _native.require_device(query_dst, 'EdgeBankPredictor: query_dst')
        pred = torch.zeros_like(query_src)
        n = query_src.numel()
        if n == 0:
            return pred
        if query_dst.numel() < n:  # the reference's zip() stops at the shorter one
            raise ValueError(f'query_dst has {query_dst.numel()} entries for {n} sources')
        out, code = self._out_like(pred)
        s, d = _ids(query_src), _ids(query_dst)
        _native.check(
            self._lib.tgmx_edgebank_query(self._block(), s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64, None, 0, None, 0,
                                          n, n, out.data_ptr(), code, self._stream()),
            'tgmx_edgebank_query',
        )  # fmt: skip
        return pred if out is pred else pred.copy_(out.view_as(pred))

    @staticmethod
    def _out_like(pred: torch.Tensor) -> Tuple[torch.Tensor, int]:
        if pred.dtype not in _OUT_DTYPES:
            raise TypeError(f'EdgeBankPredictor answers in the query dtype; supported are int32, int64, float32 and float64, got {pred.dtype}')
        out = pred if pred.is_contiguous() else torch.empty(pred.shape, dtype=pred.dtype, device=pred.device)
        return out, _OUT_DTYPES[pred.dtype]

    def query_one_vs_many(
        self, src: torch.Tensor, dst: torch.Tensor, negatives: Union[torch.Tensor, Sequence[torch.Tensor]]
    ) -> Union[torch.Tensor, List[torch.Tensor]]:
        """The evaluation loop's ``B`` calls as one launch: row ``b`` answers ``(src[b], dst[b])`` in column 0 and ``(src[b], negatives[b][m])``
        after it, with the bits ``self(src[b].repeat(1 + M), cat([dst[b:b+1], negatives[b]]))`` gives.  ``negatives`` is ``[B, M]`` (the
        result is ``[B, 1 + M]``) or a list of ``B`` 1-D tensors of any lengths, ``batch.neg_batch_list`` (the result is a list of ``B``
        tensors).  The answers have ``src``'s dtype."""
        _native.require_device(src, 'EdgeBankPredictor.query_one_vs_many: src')
        _native.require_device(dst, 'EdgeBankPredictor.query_one_vs_many: dst')
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
                _native.require_device(t, 'EdgeBankPredictor.query_one_vs_many: negatives')
            if B == 0:
                return []
            neg = _ids(torch.cat([t.reshape(-1) for t in negatives]))
            off_host = np.zeros(B + 1, dtype=np.int64)
            np.cumsum(sizes, out=off_host[1:])
            # host to device, from pinned memory so that the host does not wait: the sizes are shapes, nothing is read back
            off = torch.from_numpy(off_host).pin_memory().to(self._device, non_blocking=True)
            M, total = 0, B + int(off_host[-1])
        else:
            _native.require_device(negatives, 'EdgeBankPredictor.query_one_vs_many: negatives')
            if negatives.dim() != 2 or negatives.shape[0] != B:
                raise ValueError(f'negatives must be [B, M] with B = {B}, got {tuple(negatives.shape)}')
            neg, off = _ids(negatives), None
            M = int(negatives.shape[1])
            total = B * (M + 1)
        pred = torch.zeros(total, dtype=src.dtype, device=src.device)
        code = self._out_like(pred)[1]
        if total:
            s, d = _ids(src), _ids(dst)
            _native.check(
                self._lib.tgmx_edgebank_query(self._block(), s.data_ptr(), s.dtype == torch.int64, d.data_ptr(), d.dtype == torch.int64,
                                              neg.data_ptr() if neg.numel() else d.data_ptr(), neg.dtype == torch.int64, _native.ptr(off), M, B, total,
                                              pred.data_ptr(), code, self._stream()),
                'tgmx_edgebank_query',
            )  # fmt: skip
        if not ragged:
            return pred.view(B, M + 1) if as_rows is None else list(pred.view(B, M + 1).unbind(0))
        return list(torch.split(pred, [m + 1 for m in sizes]))

    # ---- reads from the device ------------------------------------------------------------------------------------------------------------
    def _host_state(self, words: Optional[np.ndarray] = None) -> Tuple[int, Union[int, float]]:
        """(window_end, window_start) from the state block: the start as every kernel recomputes it"""
        w = self._state.cpu().numpy() if words is None else words
        end = int(w[0])
        if self._fixed_memory:
            size = w[2:3].view(np.float32)[0]
            return end, float(np.float32(end) - size)
        return end, end - int(w[1])

    @property
    def window_start(self) -> int | float:
        """Where the memory window starts now (one read from the device): a float in fixed mode, an int otherwise."""
        return self._host_state()[1]

    @property
    def window_end(self) -> int | float:
        """The largest timestamp offered so far (one read from the device)."""
        return self._host_state()[0]

    @property
    def window_ratio(self) -> float:
        """The ``window_ratio`` the predictor was built with."""
        return self._window_ratio

    @property
    def memory(self) -> Mapping[Tuple[int, int], int]:
        """``{(src, dst): ts}`` as the reference's dict holds it after the last ``update``, built from the table by one device-to-host copy
        (for inspection, not for the loop).  In fixed mode it holds the entries whose timestamp passes the insertion test against the
        current window start: those the reference's ``_clean_up`` has not removed."""
        words = self._buf.cpu().numpy()
        slots = words[: 2 * self._capacity].reshape(self._capacity, 2)
        _, start = self._host_state(words[2 * self._capacity :])
        key, ts = slots[:, 0], slots[:, 1]
        live = key != _EMPTY
        if self._fixed_memory:
            live &= ts.astype(np.float32) >= np.float32(start)
        key, ts = key[live], ts[live]
        order = np.argsort(key, kind='stable')
        key, ts = key[order], ts[order]
        return MappingProxyType({(int(k >> 32), int(k & 0xFFFFFFFF)): int(t) for k, t in zip(key.tolist(), ts.tolist())})

    def check(self) -> None:
        """Raise ``ValueError`` for what the kernels flagged since the last check (one device-to-host read): an id outside ``[0, 2^31)``
        in an update or a query, or a table that ran full."""
        bits = int(self._status.item())
        if bits:
            self._status.zero_()
        if bits & STATUS_BAD_ID:
            raise ValueError('EdgeBankPredictor: node ids must lie in [0, 2^31); an id outside was offered or queried (it was ignored)')
        if bits & STATUS_OVERFLOW:
            raise ValueError('EdgeBankPredictor: a probe ran through the whole table (events were dropped)')

    @staticmethod
    def _check_input_data(src: Any, dst: Any, ts: Any) -> None:
        """The reference's argument checks: its order, its exception types, its messages."""
        args = (('src', src), ('dst', dst), ('ts', ts))
        describe = lambda fn: ', '.join(f'{name}: {fn(value)}' for name, value in args)
        if any(type(value) is not torch.Tensor for _, value in args):
            raise TypeError('src, dst, ts must all be Tensor, got ' + describe(type))
        if len({len(value) for _, value in args}) != 1:
            raise ValueError('mismatch shape: ' + describe(len))
        if len(src) == 0:
            raise ValueError('src, dst, ts must have at len > 1, got ' + describe(len))
