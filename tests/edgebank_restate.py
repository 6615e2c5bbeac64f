"""EdgeBankPredictor restated as a plain dictionary, in this project's own words, plus the hash of csrc/edgebank.hip mirrored in Python.

The restatement reproduces every ``g19_edgebank_*`` fixture on the CPU (``test_edgebank_cpu.py``) and is the yardstick on the GPU for cases
too large to commit.  What it states:

* fixed mode: ``size = f32(end) - (f32(end) - f32(f32(ratio) * f32(end - begin)))`` in float32, once; afterwards ``start = f32(end) - size``;
  unlimited mode: ``size = end - begin`` and ``start = end - size`` in integers;
* an update first moves ``end`` to the largest timestamp seen, then offers its events in order: one is stored iff ``ts >= start``, with ``ts``
  rounded to float32 in fixed mode; a stored event overwrites its pair's timestamp, whatever was there;
* a query hits iff the pair is stored and, in fixed mode, its timestamp (exact) ``>= start``;
* ``memory`` in fixed mode shows the entries that still pass the insertion test.

``window_arithmetic='exact'`` is NOT the reference: it is what exact arithmetic would give, and the fixture generator uses it to prove that a
fixture can tell the two apart.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Dict, Tuple

import numpy as np

MASK64 = (1 << 64) - 1
EMPTY_KEY = MASK64


def pack_key(src: int, dst: int) -> int:
    return (int(src) << 32) | int(dst)


def hash64(key: int) -> int:
    """The splitmix64 finaliser, as eb_hash in csrc/edgebank.hip."""
    x = key & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def home_slot(src: int, dst: int, capacity: int) -> int:
    """Where the probe for (src, dst) starts in a table of ``capacity`` (a power of two) slots."""
    return hash64(pack_key(src, dst)) & (capacity - 1)


class EdgeBankRestated:
    def __init__(self, src, dst, ts, memory_mode: str = 'unlimited', window_ratio: float = 0.15, pos_prob: float = 1.0,
                 window_arithmetic: str = 'float32') -> None:  # fmt: skip
        ts = np.asarray(ts).astype(np.int64)
        self.fixed = memory_mode == 'fixed'
        self.exact = window_arithmetic == 'exact'
        self.pos_prob = pos_prob
        begin, end = int(ts.min()), int(ts.max())
        self.end = end
        if not self.fixed:
            self.size = end - begin
        elif self.exact:
            self.size = Fraction(window_ratio) * (end - begin)
        else:
            f = np.float32
            start = f(f(end) - f(f(window_ratio) * f(end - begin)))
            self.size = f(f(end) - start)
        self.stored: Dict[Tuple[int, int], int] = {}
        self.update(src, dst, ts)

    @property
    def window_end(self) -> int:
        return self.end

    @property
    def window_start(self):
        if not self.fixed:
            return self.end - self.size
        if self.exact:
            return self.end - self.size
        return float(np.float32(np.float32(self.end) - self.size))

    def _insertable(self, t: int) -> bool:
        if self.fixed and not self.exact:
            return float(np.float32(t)) >= self.window_start
        return t >= self.window_start

    def update(self, src, dst, ts) -> None:
        src, dst, ts = (np.asarray(v).astype(np.int64).tolist() for v in (src, dst, ts))
        self.end = max(self.end, max(ts))
        for s, d, t in zip(src, dst, ts):
            if self._insertable(t):
                self.stored[(s, d)] = t

    def __call__(self, query_src, query_dst) -> np.ndarray:
        query_src = np.asarray(query_src)
        out = np.zeros(query_src.shape, dtype=query_src.dtype)
        start = self.window_start
        hit = np.asarray(self.pos_prob).astype(out.dtype)  # torch's cast: towards zero for the integer dtypes
        for i, (s, d) in enumerate(zip(query_src.astype(np.int64).tolist(), np.asarray(query_dst).astype(np.int64).tolist())):
            t = self.stored.get((s, d))
            if t is not None and (not self.fixed or t >= start):
                out[i] = hit
        return out

    @property
    def memory(self) -> Dict[Tuple[int, int], int]:
        if not self.fixed:
            return dict(self.stored)
        return {k: t for k, t in self.stored.items() if self._insertable(t)}

    def memory_arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        """The dictionary as sorted keys [n, 2] and their timestamps [n]: what the fixtures record."""
        items = sorted(self.memory.items())
        keys = np.array([k for k, _ in items], dtype=np.int64).reshape(-1, 2)
        return keys, np.array([t for _, t in items], dtype=np.int64)
