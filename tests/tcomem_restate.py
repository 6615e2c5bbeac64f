"""tCoMemPredictor and PopTrackPredictor restated in this project's own words, plus the pair key and home slot of csrc/tcomem.hip mirrored
in Python.

The restatement reproduces every ``g20_tcomem_*`` / ``g21_poptrack_*`` fixture on the CPU (``test_tcomem_cpu.py``) and is the yardstick on
the GPU for cases too large to commit.  What it states:

* per node a ring of the ``k`` most recent events with the node as source: an event goes to ``pos``, ``pos`` advances modulo ``k``, ``len``
  saturates at ``k``; the timestamp is rounded to float32 when stored; every event enters, whatever its timestamp;
* one counter per unordered pair, +1 per event and +2 for a self-loop (the reference increments ``[s][d]`` and ``[d][s]``);
  ``popularity[d] += 1``;
* ``size = max(f32(max(ts) - min(ts)), 1)`` of the constructor's events, once; ``end`` is the largest timestamp seen;
  ``start = f32(f32(end) - size)``; ``window_size = int(f32(f32(end) - start))``;
* the base score of a source: the sum over ring entries ``i < len`` with ``start <= ts <= f32(end)`` of
  ``exp(-(f32(end) - ts) / size) * sigmoid(popularity[dst])``; to it ``weight * (c / (1 + c))`` is added as the query's dtype decides:
  integer queries add nothing, float32 adds it rounded to float32, float64 adds it in double and rounds the sum.

The integer state and the float32 window restate bit for bit.  The scores come in two evaluations from the same state: ``scores`` in
float32 (numpy's ``exp`` and summation order, so near the reference's bits, not equal to them) and ``scores64`` with every term, sum and the
co-occurrence term in float64.  ``scores64`` is the record the float32 answers of the reference, of this restatement and of the kernel are
measured against.

``arithmetic='exact'`` is NOT the reference: timestamps are stored unrounded and the window is ``[end - size, end]`` exactly.  The fixture
generator uses it to prove that a fixture can tell the two apart.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from edgebank_restate import EMPTY_KEY, hash64  # noqa: F401  (the table is EdgeBank's: the same hash, the same empty key)

F = np.float32
INTEGER_QUERIES = ('int32', 'int64')


def pair_key(src: int, dst: int) -> int:
    """tc_key in csrc/tcomem.hip: the smaller id in the upper half."""
    a, b = (int(src), int(dst)) if src < dst else (int(dst), int(src))
    return (a << 32) | b


def home_slot(src: int, dst: int, capacity: int) -> int:
    """Where the probe for the unordered pair starts in a table of ``capacity`` (a power of two) slots."""
    return hash64(pair_key(src, dst)) & (capacity - 1)


def rel_err(got, ref64) -> float:
    """max |got - ref| / max(1, |ref|)"""
    got, ref64 = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref64, dtype=np.float64).reshape(-1)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref64) / np.maximum(1.0, np.abs(ref64))))


class TCoMemRestated:
    def __init__(self, src, dst, ts, num_nodes: int, k: int = 50, co_occurrence_weight: float = 0.8, integer_queries_add: bool = False,
                 arithmetic: str = 'float32') -> None:  # fmt: skip
        ts = np.asarray(ts).astype(np.int64)
        self.exact = arithmetic == 'exact'
        self.N, self.k, self.weight = int(num_nodes), int(k), float(co_occurrence_weight)
        self.integer_queries_add = integer_queries_add  # NOT the reference: integer queries take the float32 rule
        self.end = int(ts.max())
        self.size = max(F(int(ts.max()) - int(ts.min())), F(1.0))
        if self.exact:
            self.size = max(int(ts.max()) - int(ts.min()), 1)
        self.recent_ts = np.full((self.N, self.k), -np.inf, dtype=np.float64 if self.exact else F)
        self.recent_dst = np.full((self.N, self.k), -1, dtype=np.int64)
        self.pos = np.zeros(self.N, dtype=np.int64)
        self.len = np.zeros(self.N, dtype=np.int64)
        self.pop = np.zeros(self.N, dtype=np.int64)
        self.counts: Dict[Tuple[int, int], int] = {}  # (min, max) -> count
        self.update(src, dst, ts)

    # ---- the window -----------------------------------------------------------------------------------------------------------------------
    @property
    def window_end(self) -> int:
        return self.end

    @property
    def window_start(self) -> float:
        if self.exact:
            return float(self.end - self.size)
        return float(F(F(self.end) - self.size))

    @property
    def window_size(self) -> int:
        return int(F(F(self.end) - F(self.window_start)))

    # ---- the state ------------------------------------------------------------------------------------------------------------------------
    def update(self, src, dst, ts) -> None:
        src, dst, ts = (np.asarray(v).astype(np.int64).tolist() for v in (src, dst, ts))
        self.end = max(self.end, max(ts))
        for s, d, t in zip(src, dst, ts):
            if not (0 <= s < self.N and 0 <= d < self.N):
                raise IndexError((s, d))
            p = self.pos[s]
            self.recent_ts[s, p] = t if self.exact else F(t)
            self.recent_dst[s, p] = d
            self.pos[s] = (p + 1) % self.k
            self.len[s] = min(self.len[s] + 1, self.k)
            key = (min(s, d), max(s, d))
            self.counts[key] = self.counts.get(key, 0) + (2 if s == d else 1)
            self.pop[d] += 1

    def count(self, s: int, d: int) -> int:
        return self.counts.get((min(s, d), max(s, d)), 0)

    def nested_counts(self) -> Dict[int, Dict[int, int]]:
        """both directions, as the reference's node_to_co_occurrence"""
        out: Dict[int, Dict[int, int]] = {}
        for (a, b), c in sorted(self.counts.items()):
            out.setdefault(a, {})[b] = c
            out.setdefault(b, {})[a] = c
        return out

    def count_arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        """The counts as sorted unordered pairs [n, 2] (smaller id first) and their counts [n]: what the fixtures record."""
        items = sorted(self.counts.items())
        return np.array([k for k, _ in items], dtype=np.int64).reshape(-1, 2), np.array([c for _, c in items], dtype=np.int64)

    # ---- the scores -----------------------------------------------------------------------------------------------------------------------
    def _mask(self, s: int) -> np.ndarray:
        ts = self.recent_ts[s]
        if self.exact:
            return (np.arange(self.k) < self.len[s]) & (ts >= self.window_start) & (ts <= self.end)
        return (np.arange(self.k) < self.len[s]) & (ts >= F(self.window_start)) & (ts <= F(self.end))

    def base(self, s: int) -> np.float32:
        m = self._mask(s)
        ts, pop = self.recent_ts[s][m], self.pop[self.recent_dst[s][m]].astype(F)
        decay = np.exp(-(F(self.end) - ts) / self.size)
        return F(np.sum(decay * (F(1) / (F(1) + np.exp(-pop))), dtype=F))

    def base64(self, s: int) -> float:
        m = self._mask(s)
        ts, pop = self.recent_ts[s][m].astype(np.float64), self.pop[self.recent_dst[s][m]].astype(np.float64)
        decay = np.exp(-(float(F(self.end)) - ts) / float(self.size))
        return float(np.sum(decay / (1.0 + np.exp(-pop))))

    def _term(self, s: int, d: int, dtype: str) -> float:
        if dtype in INTEGER_QUERIES and not self.integer_queries_add:
            return 0.0
        c = self.count(s, d)
        return self.weight * (c / (1 + c))

    def scores(self, query_src, query_dst, dtype: str) -> np.ndarray:
        """float32, as the reference answers queries handed over in `dtype`"""
        qs, qd = np.asarray(query_src).astype(np.int64).tolist(), np.asarray(query_dst).astype(np.int64).tolist()
        base = {s: self.base(s) for s in set(qs)}
        out = np.zeros(len(qs), dtype=F)
        for i, (s, d) in enumerate(zip(qs, qd)):
            t = self._term(s, d, dtype)
            out[i] = F(np.float64(base[s]) + t) if dtype == 'float64' else base[s] + F(t)
        return out

    def scores64(self, query_src, query_dst, dtype: str) -> np.ndarray:
        """the same answers with every term, sum and the co-occurrence term in float64"""
        qs, qd = np.asarray(query_src).astype(np.int64).tolist(), np.asarray(query_dst).astype(np.int64).tolist()
        base = {s: self.base64(s) for s in set(qs)}
        return np.array([base[s] + self._term(s, d, dtype) for s, d in zip(qs, qd)], dtype=np.float64)


class PopTrackRestated:
    """per node: add 1.0f once per occurrence as a destination, then multiply by f32(decay)"""

    def __init__(self, src, dst, ts, num_nodes: int, k: int = 50, decay: float = 0.9) -> None:
        self.popularity = np.zeros(int(num_nodes), dtype=F)
        self.decay = F(decay)
        self.update(src, dst, ts)

    def update(self, src, dst, ts) -> None:
        for d in np.asarray(dst).astype(np.int64).tolist():
            self.popularity[d] = self.popularity[d] + F(1.0)
        self.popularity *= self.decay

    def __call__(self, query_src, query_dst) -> np.ndarray:
        return self.popularity[np.asarray(query_dst).astype(np.int64)]
