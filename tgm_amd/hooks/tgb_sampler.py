"""TGB's pre-generated evaluation negatives (the reference's ``tgm/hooks/negatives/tgb_sampler.py``): ``neg`` = the sorted unique negative
destinations of a batch (int32), ``neg_batch_list`` = one int32 tensor of candidates per positive edge, ``neg_time`` = one int64 time per
entry of ``neg``, drawn by the reference's own expression (a generator seeded 0, ``randint`` over the batch's time span).

The reference answers a batch with a dictionary lookup, an ``int()`` per negative and a ``torch.tensor(list)`` per positive, then
``torch.cat``, ``torch.unique`` and two ``.item()``.  The evaluation set of a split never changes, so on a ROCm device it is uploaded once
(``csrc/tgbneg.hip``): an open-addressing table from the key tuple to a row of one int32 pool.  A batch is then two launches -- a probe that
copies every positive's row into a padded ``[B, Qpad]`` matrix and marks its ids in a bitmap, and an ordered compaction of that bitmap --
and ONE read of ``[n_unique, min(edge_time), max(edge_time), first missing position]`` with the ``B`` row lengths.

Where the evaluation set comes from:

* the reference's constructor ``(dataset_name, split_mode, ...)`` needs the ``tgb`` package and builds its sampler exactly as the reference
  does (kept as ``neg_sampler``).  On the first device call the table is built from ``neg_sampler.eval_set[split_mode]`` if that is a
  ``dict`` from integer tuples of the expected arity to integer arrays, AND up to 64 of its own keys, sent through
  ``neg_sampler.query_batch``, come back as the rows the table holds.  Otherwise -- a sampler whose ``query_batch`` does more than a lookup,
  a mock -- the hook *delegates*: ``query_batch`` is called as in the reference, its answer goes to the device as one padded matrix, and the
  same compaction runs.  A wrong guess about ``tgb``'s internals costs speed, never correctness;
* :meth:`from_eval_set` (extension) takes the mapping itself; no ``tgb`` needed.

Host tensors (``dg.device`` is the CPU) run the same definitions in numpy, equal exactly.  A positive edge that is not in the evaluation set
raises the reference's ``ValueError`` (``... `pip install --upgrade py-tgb` ``), chained from one that names the batch position and the edge
of the first missing positive; the next call is unaffected.

The matrix, ``neg`` and the lengths of a call are new tensors (a batch may be kept while the next one is made); the table, the bitmap and the
scratch words are the hook's and are regrown only when they must.
"""
from __future__ import annotations

import ctypes
import logging
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..core import DGBatch, DGraph
from ..core.neg_batch_list import NegBatchList
from .base import StatelessHook
from .registry import hook

logger = logging.getLogger(__name__)

_FIELDS = {'src': 0, 'dst': 1, 'time': 2, 'edge_type': 3}  # tgmx_tgbneg_t.field
_ATTRS = ('edge_src', 'edge_dst', 'edge_time', 'edge_type')
_NONE_MISSING = 0x7FFFFFFF
_INT = (torch.int32, torch.int64)


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def flatten_eval_set(eval_set: Any, arity: int) -> Optional[Dict[str, Any]]:
    """``{key tuple: negatives}`` as the arrays of ``tgmx_tgbneg_t``: ``keys [P, 4]`` int64 (unused fields 0), ``indptr [P + 1]`` int64 (every
    row starts at a multiple of four), ``rowlen [P]`` int32, ``pool`` int32 with -1 in the gaps; ``qpad`` and ``max_id``.  ``None`` when the
    object is not such a mapping (the caller then delegates): not a non-empty dict, a key that is no tuple of ``arity`` integers, a value that
    is no 1-D integer array with ids in ``[0, 2^31 - 1)``."""
    if not isinstance(eval_set, dict) or not eval_set or not 1 <= arity <= 4:
        return None
    P = len(eval_set)
    keys = np.zeros((P, 4), dtype=np.int64)
    rows: List[np.ndarray] = []
    try:
        for p, (k, v) in enumerate(eval_set.items()):
            if not isinstance(k, tuple) or len(k) != arity or not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in k):
                return None
            keys[p, :arity] = k
            a = np.asarray(v)
            if a.ndim != 1 or (a.size and a.dtype.kind not in 'iu'):
                return None
            rows.append(a)
    except (OverflowError, TypeError, ValueError):
        return None
    lens = np.fromiter((a.size for a in rows), dtype=np.int64, count=P)
    indptr = np.zeros(P + 1, dtype=np.int64)
    np.cumsum((lens + 3) & ~3, out=indptr[1:])
    if indptr[-1] >= 1 << 40:
        return None
    pool = np.full(int(indptr[-1]), -1, dtype=np.int32)
    max_id = 0
    for p, a in enumerate(rows):
        if a.size:
            lo, hi = int(a.min()), int(a.max())
            if lo < 0 or hi >= (1 << 31) - 1:
                return None
            max_id = max(max_id, hi)
            pool[indptr[p] : indptr[p] + a.size] = a
    return dict(keys=keys, indptr=indptr, rowlen=lens.astype(np.int32), pool=pool, qpad=max(4, _round_up(int(lens.max()), 4)), max_id=max_id)


def pad_rows(rows: Sequence[Any]) -> Tuple[np.ndarray, np.ndarray]:
    """A list of id lists as the padded matrix ``[B, Qpad]`` int32 (-1 behind every row) and its lengths."""
    arrs = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
    lens = np.fromiter((a.size for a in arrs), dtype=np.int32, count=len(arrs))
    qpad = max(4, _round_up(int(lens.max()) if len(arrs) else 0, 4))
    matrix = np.full((len(arrs), qpad), -1, dtype=np.int32)
    for b, a in enumerate(arrs):
        if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
            raise ValueError(f'negative candidates of batch position {b} do not fit int32')
        matrix[b, : a.size] = a
    return matrix, lens


class _DeviceState:
    """What one device holds for one hook: the table (if any), the bitmap and the scratch words."""

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self.table: Optional[Dict[str, torch.Tensor]] = None
        self.capacity = 0
        self.qpad = 4
        self.bitmap: Optional[torch.Tensor] = None
        self.block_counts: Optional[torch.Tensor] = None
        self.first_missing = torch.full((1,), _NONE_MISSING, dtype=torch.int32, device=device)
        self.gen = torch.Generator(device=device)

    def reserve_bitmap(self, max_id: int) -> None:
        lib = _native.load()
        one_wg, chunk = int(lib.tgmx_tgbneg_limit(1)), int(lib.tgmx_tgbneg_limit(2))
        words = max_id // 32 + 1
        words = _round_up(words, chunk) if words > one_wg else _round_up(words, 4)
        if self.bitmap is None or self.bitmap.numel() < words:  # every call leaves the bitmap zero: a larger one replaces it as it is
            self.bitmap = torch.zeros(words, dtype=torch.int32, device=self.device)
            self.block_counts = torch.zeros(max(1, words // chunk), dtype=torch.int32, device=self.device)

    def block(self, field: Sequence[int]) -> _native.TgbNeg:
        t = self.table or {}
        P = lambda name: t[name].data_ptr() if name in t else 0
        return _native.TgbNeg(P('keys'), P('indptr'), P('rowlen'), P('pool'), t['keys'].shape[0] if t else 0, t['pool'].numel() if t else 0, P('slots'),
                              self.capacity, self.bitmap.data_ptr(), self.bitmap.numel(), self.first_missing.data_ptr(), self.block_counts.data_ptr(),
                              self.block_counts.numel(), self.qpad, (ctypes.c_int32 * 4)(*field), 0)  # fmt: skip


@hook
class TGBNegativeEdgeSamplerBase(StatelessHook):
    """Base class for TGB pre-generated negative edge sampler hooks.

    Args:
        dataset_name (str): The name of the TGB dataset.
        split_mode (str): The split mode to use for sampling, either 'val' or 'test'.
        id (str | None): A unique identifier for the hook.

    Attributes produced:
        neg (Tensor[int32]): Unique negative destination node ids across the batch, ascending.
        neg_batch_list (NegBatchList): Per-edge negative candidate tensors (int32), aligned with ``batch.edge_src``.
        neg_time (Tensor[int64]): Randomly sampled timestamps for each negative, drawn uniformly from
            ``[batch.edge_time.min(), batch.edge_time.max()]`` with a fixed seed for reproducibility.
    """

    _dataset_prefix: str
    _default_key: Tuple[str, ...] = ('src', 'dst', 'time')
    _with_edge_type = False

    def __init__(self, dataset_name: str, split_mode: str, id: str | None = None) -> None:
        super().__init__()
        if split_mode not in ['val', 'test']:
            raise ValueError(f'split_mode must be "val" or "test", got: {split_mode}')

        try:
            from tgb.utils.info import DATA_VERSION_DICT, PROJ_DIR
        except ImportError:
            raise ImportError(f'TGB required for {self.__class__.__name__}, try `pip install py-tgb`')

        if not dataset_name.startswith(f'{self._dataset_prefix}-'):
            raise ValueError(
                f'TGBNegativeEdgeSamplerHook should only be registered for "{self._dataset_prefix}-xxx" datasets, but got: {dataset_name}'
            )

        neg_sampler = self._build_sampler(dataset_name)

        root = Path(PROJ_DIR + 'datasets') / dataset_name.replace('-', '_')
        if DATA_VERSION_DICT.get(dataset_name, 1) > 1:
            version_suffix = f'_v{DATA_VERSION_DICT[dataset_name]}'
        else:
            version_suffix = ''
        ns_fname = root / f'{dataset_name}_{split_mode}_ns{version_suffix}.pkl'
        logger.debug('Loading %s split (neg_sampler.load_eval_set) for dataset: %s from file: %s', split_mode, dataset_name, ns_fname)
        neg_sampler.load_eval_set(fname=str(ns_fname), split_mode=split_mode)

        self.neg_sampler = neg_sampler
        self.split_mode = split_mode
        self._id = id
        self._init_native(None, self._default_key, None)
        self.__post_init__()

    @classmethod
    def from_eval_set(cls, eval_set: Dict[tuple, Any], split_mode: str = 'val', key: Optional[Sequence[str]] = None, id: Optional[str] = None,
                      _capacity: Optional[int] = None, **id_range: Any) -> 'TGBNegativeEdgeSamplerBase':  # fmt: skip
        """A hook over the evaluation set itself (extension; ``tgb`` is not needed): ``eval_set`` maps a tuple of integers to the 1-D integer
        array of that positive edge's negative destinations (a ``{split: mapping}`` dict, as a TGB sampler's ``eval_set`` is, is also taken).
        ``key`` names the batch fields in the tuples' order, out of ``'src'``, ``'dst'``, ``'time'``, ``'edge_type'`` (default: the class's TGB
        order).  ``id_range``: the class's own id-range arguments (all of them or none), checked as its constructor checks them."""
        if split_mode not in ['val', 'test']:
            raise ValueError(f'split_mode must be "val" or "test", got: {split_mode}')
        self = cls.__new__(cls)
        StatelessHook.__init__(self)
        if id_range:
            self._check_id_range(**id_range)
        key = tuple(cls._default_key if key is None else key)
        if not 1 <= len(key) <= 4 or len(set(key)) != len(key) or any(k not in _FIELDS for k in key):
            raise ValueError(f'key must name one to four distinct fields out of {sorted(_FIELDS)}, got: {key}')
        if 'edge_type' in key and not cls._with_edge_type:
            raise ValueError(f"{cls.__name__} does not require 'edge_type'; use the thgl / tkgl hook for keys with it")
        if isinstance(eval_set, dict) and isinstance(eval_set.get(split_mode), dict):
            eval_set = eval_set[split_mode]
        flat = flatten_eval_set(eval_set, len(key))
        if flat is None:
            raise ValueError(f'eval_set must be a non-empty dict from tuples of {len(key)} integers {key} to 1-D integer arrays of ids in [0, 2^31 - 1)')
        if _capacity is not None and (_capacity <= len(eval_set) or _capacity & (_capacity - 1)):
            raise ValueError(f'_capacity must be a power of two above the {len(eval_set)} keys, got: {_capacity}')
        self.neg_sampler = None
        self.split_mode = split_mode
        self._id = id
        self._init_native(eval_set, key, _capacity)
        self._flat = flat
        self.__post_init__()
        return self

    def _check_id_range(self) -> None:
        pass

    def _init_native(self, eval_set: Optional[dict], key: Tuple[str, ...], capacity: Optional[int]) -> None:
        self._eval: Optional[dict] = eval_set  # from_eval_set: the mapping the host path looks keys up in
        self._key = key
        self._field = [_FIELDS[k] for k in key] + [-1] * (4 - len(key))
        self._capacity = capacity
        self._flat: Optional[Dict[str, Any]] = None
        self._delegating = False  # for good once set (a sampler object only)
        self._dev: Dict[torch.device, _DeviceState] = {}

    # ---- what the subclasses say ------------------------------------------------------------------------------------------------------------
    def _build_sampler(self, dataset_name: str) -> Any:
        """Instantiate and return the TGB negative sampler. Must be implemented by subclasses."""
        raise NotImplementedError

    def _query_batch(self, batch: DGBatch) -> list:
        """Query the sampler for a batch. Must be implemented by subclasses."""
        raise NotImplementedError

    def _sampler_args(self, fields: Sequence[Any]) -> tuple:
        """(src, dst, time, edge_type) as ``neg_sampler.query_batch``'s positional arguments."""
        return tuple(fields) if self._with_edge_type else tuple(fields[:3])

    # ---- the call ---------------------------------------------------------------------------------------------------------------------------
    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        B = batch.edge_src.size(0)
        device = dg.device
        if B == 0:
            neg = torch.empty(0, dtype=torch.int32, device=device)
            neg_time = torch.empty(0, dtype=torch.int64, device=device)
            neg_list: list = []
        else:
            try:
                if device.type == 'cuda':
                    neg, neg_list, tmin, tmax = self._call_device(batch, B, device)
                else:
                    neg, neg_list, tmin, tmax = self._call_host(batch, B, device)
            except ValueError as e:
                raise ValueError(
                    f'{self._dataset_prefix.upper()} Negative sampling failed for split_mode={self.split_mode}. Try updating your TGB package: `pip install --upgrade py-tgb`'
                ) from e
            # the reference's expression: on a given device the same generator state gives the same times
            gen = self._state(device).gen if device.type == 'cuda' else torch.Generator(device=device)
            gen.manual_seed(0)
            neg_time = torch.randint(tmin, tmax + 1, (neg.size(0),), device=device, generator=gen)

        self.add_batch_attribute(batch, 'neg', neg)
        self.add_batch_attribute(batch, 'neg_batch_list', neg_list)
        self.add_batch_attribute(batch, 'neg_time', neg_time)
        return batch

    def _missing(self, batch: DGBatch, b: int) -> ValueError:
        edge = ', '.join(f'{a[5:]}={int(getattr(batch, a)[b])}' for a in _ATTRS[: 4 if self._with_edge_type else 3])
        return ValueError(f'no negatives for the positive edge at batch position {b}: ({edge}) is not a key of the {self.split_mode} evaluation set')

    def _rows(self, batch: DGBatch) -> Sequence[Any]:
        """One id sequence per positive, on the host: ``query_batch`` of a sampler object, else lookups in the mapping."""
        if self.neg_sampler is not None:
            return self._query_batch(batch)
        cols = [getattr(batch, _ATTRS[f]).tolist() for f in self._field[: len(self._key)]]
        rows = []
        for b, k in enumerate(zip(*cols)):
            row = self._eval.get(k)
            if row is None:
                raise self._missing(batch, b)
            rows.append(row)
        return rows

    def _call_host(self, batch: DGBatch, B: int, device: torch.device):
        matrix_h, lens = pad_rows(self._rows(batch))
        valid = np.arange(matrix_h.shape[1])[None, :] < lens[:, None]
        neg = torch.from_numpy(np.unique(matrix_h[valid]).astype(np.int32)).to(device)
        matrix = torch.from_numpy(matrix_h).to(device)
        neg_list = NegBatchList(matrix, torch.from_numpy(lens).to(device), lens.tolist())
        return neg, neg_list, int(batch.edge_time.min().item()), int(batch.edge_time.max().item())

    # ---- the device path --------------------------------------------------------------------------------------------------------------------
    def _state(self, device: torch.device) -> _DeviceState:
        st = self._dev.get(device)
        if st is None:
            st = self._dev[device] = _DeviceState(device)
        return st

    def _table(self, st: _DeviceState) -> bool:
        """True when ``st`` holds (now, at the latest) the table of the evaluation set; False: delegate."""
        if st.table is not None:
            return True
        if self._delegating:
            return False
        if self._flat is None and self.neg_sampler is not None:
            eval_set = getattr(self.neg_sampler, 'eval_set', None)
            split = eval_set.get(self.split_mode) if isinstance(eval_set, dict) else None
            self._flat = flatten_eval_set(split, len(self._key))
            if self._flat is None:
                self._delegating = True
                return False
            self._eval = split
        flat = self._flat
        lib = _native.load()
        P = flat['keys'].shape[0]
        capacity = 64
        while capacity < 2 * P:
            capacity <<= 1
        if self._capacity is not None:  # from_eval_set checked it
            capacity = int(self._capacity)
        dev = st.device
        table = {k: torch.from_numpy(flat[k]).to(dev) for k in ('keys', 'indptr', 'rowlen', 'pool')}
        if table['pool'].numel() == 0:  # every row empty: the pool still has an address
            table['pool'] = torch.full((4,), -1, dtype=torch.int32, device=dev)
        table['slots'] = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
        st.table, st.capacity, st.qpad = table, capacity, flat['qpad']
        st.reserve_bitmap(flat['max_id'])
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.tgmx_tgbneg_build(ctypes.byref(st.block(self._field)), status.data_ptr(), _native.stream_ptr(dev.index)), 'tgmx_tgbneg_build')
        bits = int(status.item())  # once per hook and device
        if bits:
            st.table = None
            raise RuntimeError(f'tgmx_tgbneg_build: status {bits} (1: two rows with one key, 2: no free slot) for {P} keys in {capacity} slots')
        if self.neg_sampler is not None and not self._self_check(st):
            st.table, self._delegating = None, True
            return False
        return True

    def _self_check(self, st: _DeviceState) -> bool:
        """Up to 64 of the set's own keys through ``neg_sampler.query_batch`` against the table's rows.  A field the key does not hold is 0,
        but ``dst`` is the row's first negative: a sampler that filters the positive destination out of its answer then disagrees."""
        flat = self._flat
        P = flat['keys'].shape[0]
        pick = np.unique(np.linspace(0, P - 1, min(P, 64)).astype(np.int64))
        fields = [np.zeros(len(pick), dtype=np.int64) for _ in range(4)]
        for j, f in enumerate(self._field[: len(self._key)]):
            fields[f] = flat['keys'][pick, j].copy()
        if 'dst' not in self._key:
            fields[1] = np.array([flat['pool'][flat['indptr'][p]] if flat['rowlen'][p] else 0 for p in pick], dtype=np.int64)
        probe = _Fields(*(torch.from_numpy(f) for f in fields))
        try:
            answers = self.neg_sampler.query_batch(*self._sampler_args([probe.edge_src, probe.edge_dst, probe.edge_time, probe.edge_type]), split_mode=self.split_mode)
            ok = len(answers) == len(pick)
            for p, ans in zip(pick, answers):
                want = flat['pool'][flat['indptr'][p] : flat['indptr'][p] + flat['rowlen'][p]]
                ok = ok and np.array_equal(np.asarray(ans, dtype=np.int64).reshape(-1), want.astype(np.int64))
        except ValueError as e:
            logger.warning('%r: neg_sampler.query_batch refused keys of its own evaluation set (%s); delegating every batch to it', self, e)
            return False
        if not ok:
            logger.warning('%r: neg_sampler.query_batch answers differently from its evaluation set; delegating every batch to it', self)
        return ok

    def _call_device(self, batch: DGBatch, B: int, device: torch.device):
        lib = _native.load()
        st = self._state(device)
        time = batch.edge_time
        if time.dtype not in _INT or not time.is_contiguous():
            time = time.to(torch.int64).contiguous()
        stream = _native.stream_ptr(device.index)
        words = (B + 1) // 2
        if self._table(st):
            cols = []
            for a in _ATTRS:
                v = getattr(batch, a, None) if (a != 'edge_type' or self._with_edge_type) else None
                if v is not None and (v.dtype not in _INT or not v.is_contiguous()):
                    v = v.to(torch.int64).contiguous()
                cols.append(v)
            cols[2] = time
            qpad = st.qpad
            matrix = torch.empty((B, qpad), dtype=torch.int32, device=device)
            neg_cap = min(B * qpad, 32 * st.bitmap.numel())
            neg_buf = torch.empty(neg_cap, dtype=torch.int32, device=device)
            stats = torch.empty(4 + words, dtype=torch.int64, device=device)
            args = []
            for v in cols:
                args += [_native.ptr(v), int(v is not None and v.dtype == torch.int64)]
            _native.check(lib.tgmx_tgbneg_query(ctypes.byref(st.block(self._field)), *args, B, matrix.data_ptr(), neg_buf.data_ptr(), neg_cap,
                                                stats.data_ptr(), stream), 'tgmx_tgbneg_query')  # fmt: skip
            host = stats.cpu().numpy()  # the call's one read
            n, tmin, tmax, missing = (int(x) for x in host[:4])
            if missing >= 0:
                raise self._missing(batch, missing)
            host_lens = host[4:].view(np.int32)[:B].tolist()
            lengths = stats[4:].view(torch.int32)[:B]
        else:
            matrix_h, lens = pad_rows(self._rows(batch))
            qpad = matrix_h.shape[1]
            valid = matrix_h[np.arange(qpad)[None, :] < lens[:, None]]
            if valid.size and valid.min() < 0:
                raise ValueError('neg_sampler.query_batch answered a negative node id')
            st.qpad = qpad
            st.reserve_bitmap(int(valid.max()) if valid.size else 0)
            staged = torch.from_numpy(np.concatenate([matrix_h.reshape(-1), lens])).pin_memory().to(device, non_blocking=True)  # one copy
            matrix, lengths = staged[: B * qpad].view(B, qpad), staged[B * qpad :]
            neg_cap = min(B * qpad, 32 * st.bitmap.numel())
            neg_buf = torch.empty(neg_cap, dtype=torch.int32, device=device)
            stats = torch.empty(4, dtype=torch.int64, device=device)
            _native.check(lib.tgmx_tgbneg_unique(ctypes.byref(st.block(self._field)), matrix.data_ptr(), B, time.data_ptr(), int(time.dtype == torch.int64),
                                                 neg_buf.data_ptr(), neg_cap, stats.data_ptr(), stream), 'tgmx_tgbneg_unique')  # fmt: skip
            n, tmin, tmax, _ = (int(x) for x in stats.cpu().numpy())  # the call's one read
            host_lens = lens.tolist()
        return neg_buf[:n], NegBatchList(matrix, lengths, host_lens), tmin, tmax


class _Fields:
    """The four batch vectors under their attribute names (the self-check's probe batch)."""

    def __init__(self, src, dst, time, edge_type) -> None:
        self.edge_src, self.edge_dst, self.edge_time, self.edge_type = src, dst, time, edge_type


@hook
class TGBNegativeEdgeSamplerHook(TGBNegativeEdgeSamplerBase):
    """Load data from DGraph using pre-generated TGB negative samples.
    Make sure to perform `dataset.load_val_ns()` or `dataset.load_test_ns()` before using this hook.

    Args:
        dataset_name (str): The name of the TGB dataset to produce sampler for.
        split_mode (str): The split mode to use for sampling, either 'val' or 'test'.
        id (str): A unique identifier for the hook. The hook's name and all attributes it produces will be suffixed with this `id`.

    Key words: negative sampler, evaluation, tgbl, link prediction.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time'}
    _cls_produces = {'neg', 'neg_batch_list', 'neg_time'}
    _dataset_prefix = 'tgbl'

    def _build_sampler(self, dataset_name: str) -> Any:
        try:
            from tgb.linkproppred.negative_sampler import NegativeEdgeSampler
        except ImportError:
            raise ImportError(f'TGB required for {self.__class__.__name__}, try `pip install py-tgb`')
        return NegativeEdgeSampler(dataset_name=dataset_name)

    def _query_batch(self, batch: DGBatch) -> list:
        return self.neg_sampler.query_batch(batch.edge_src, batch.edge_dst, batch.edge_time, split_mode=self.split_mode)


@hook
class TGBTHGNegativeEdgeSamplerHook(TGBNegativeEdgeSamplerBase):
    """Load data from DGraph using pre-generated TGB negative samples for heterogeneous graph.
    Make sure to perform `dataset.load_val_ns()` or `dataset.load_test_ns()` before using this hook.

    Args:
        dataset_name (str): The name of the TGB dataset to produce sampler for.
        split_mode (str): The split mode to use for sampling, either 'val' or 'test'.
        first_node_id (int): identity of the first node
        last_node_id (int): identity of the last destination node
        node_type (Tensor): the node type of each node
        id (str): A unique identifier for the hook. The hook's name and all attributes it produces will be suffixed with this `id`.

    Key words: heterogeneous graph, link prediction, evaluation, negative sampler, thgl.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time', 'edge_type'}
    _cls_produces = {'neg', 'neg_batch_list', 'neg_time'}
    _dataset_prefix = 'thgl'
    _default_key = ('time', 'src', 'edge_type')
    _with_edge_type = True

    def __init__(self, dataset_name: str, split_mode: str, first_node_id: int, last_node_id: int, node_type: torch.Tensor,
                 id: str | None = None) -> None:  # fmt: skip
        self._check_id_range(first_node_id, last_node_id, node_type)
        super().__init__(dataset_name, split_mode, id)

    def _check_id_range(self, first_node_id: int, last_node_id: int, node_type: torch.Tensor) -> None:
        if first_node_id < 0 or last_node_id < 0:
            raise ValueError('First and last ID of node must be positive')
        if node_type is None:
            raise ValueError('Node type must not be None')
        if node_type.shape[0] < last_node_id:
            raise ValueError(f'last_node_id {last_node_id} must be within node_type')
        self._first_node_id = first_node_id
        self._last_node_id = last_node_id
        self._node_type = node_type

    def _build_sampler(self, dataset_name: str) -> Any:
        try:
            from tgb.linkproppred.thg_negative_sampler import THGNegativeEdgeSampler
        except ImportError:
            raise ImportError(f'TGB required for {self.__class__.__name__}, try `pip install py-tgb`')
        return THGNegativeEdgeSampler(dataset_name=dataset_name, first_node_id=self._first_node_id, last_node_id=self._last_node_id,
                                      node_type=self._node_type.numpy())  # fmt: skip

    def _query_batch(self, batch: DGBatch) -> list:
        return self.neg_sampler.query_batch(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_type, split_mode=self.split_mode)


@hook
class TGBTKGNegativeEdgeSamplerHook(TGBNegativeEdgeSamplerBase):
    """Load data from DGraph using pre-generated TGB negative samples for knowledge graph.
    Make sure to perform `dataset.load_val_ns()` or `dataset.load_test_ns()` before using this hook.

    Args:
        dataset_name (str): The name of the TGB dataset to produce sampler for.
        split_mode (str): The split mode to use for sampling, either 'val' or 'test'.
        first_dst_id (int): identity of the first destination node
        last_dst_id (int): identity of the last destination node
        id (str): A unique identifier for the hook. The hook's name and all attributes it produces will be suffixed with this `id`.

    Key words: knowledge graph, link prediction, evaluation, negative sampler, tkgl.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time', 'edge_type'}
    _cls_produces = {'neg', 'neg_batch_list', 'neg_time'}
    _dataset_prefix = 'tkgl'
    _default_key = ('time', 'src', 'edge_type')
    _with_edge_type = True

    def __init__(self, dataset_name: str, split_mode: str, first_dst_id: int, last_dst_id: int, id: str | None = None) -> None:
        self._check_id_range(first_dst_id, last_dst_id)
        super().__init__(dataset_name, split_mode, id)

    def _check_id_range(self, first_dst_id: int, last_dst_id: int) -> None:
        if first_dst_id < 0 or last_dst_id < 0:
            raise ValueError('First and last ID of node must be positive')
        self._first_dst_id = first_dst_id
        self._last_dst_id = last_dst_id

    def _build_sampler(self, dataset_name: str) -> Any:
        try:
            from tgb.linkproppred.tkg_negative_sampler import TKGNegativeEdgeSampler
        except ImportError:
            raise ImportError(f'TGB required for {self.__class__.__name__}, try `pip install py-tgb`')
        return TKGNegativeEdgeSampler(dataset_name=dataset_name, first_dst_id=self._first_dst_id, last_dst_id=self._last_dst_id)

    def _query_batch(self, batch: DGBatch) -> list:
        return self.neg_sampler.query_batch(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_type, split_mode=self.split_mode)
