"""Negative destinations for link prediction: random ids, and draws from each source's own past destinations.

RandomNegativeEdgeSamplerHook:

Same contract as tgm/hooks/negatives/sampler.py:15-65: ``neg`` = uniform int32
ids in ``[low, high)`` (one per positive edge, times ``neg_ratio``), ``neg_time``
= a copy of the batch's edge times; it produces the third seed group the neighbor sampler consumes.
On a ROCm device both outputs come from one ``tgmx_random_negatives`` launch (counter-based generator seeded from
``seed`` or ``torch.initial_seed()``: reproducible under ``torch.manual_seed``, but not torch's Philox stream); host
tensors use ``torch.randint`` like the reference.

HistoricalNegativeEdgeSamplerHook (tgm/hooks/negatives/sampler.py:68-238): ``neg[i]`` = one past event of ``edge_src[i]`` as a source, drawn
uniformly, that event's destination; -1 (and ``valid_neg_mask`` False) where the source has none.  The draw is DEFINED, for call c (counted from
1 over the hook's life) and a source s with n past events in arrival order, as ``history_s[umulhi32(counter_u32(seed, c, s), n)]`` with the
counter-based generator of csrc/common.h, so device and host tensors give the same ids bit for bit.  On a ROCm device a batch is one
``tgmx_histneg_step`` call (csrc/histneg.hip: O(1) expected work per draw and per appended event, nothing read back); host tensors run the same
definition over Python lists.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import torch

from .. import _native
from ..constants import PADDED_NODE_ID
from ..core import DGBatch, DGraph
from .base import StatefulHook, StatelessHook
from .registry import hook


@hook
class RandomNegativeEdgeSamplerHook(StatelessHook):
    """Random sampling of negative edges for dynamic link prediction.

    Key words: negative sampler, random, uniform, training, link prediction.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time'}
    _cls_produces = {'neg', 'neg_time'}

    def __init__(
        self,
        low: int,
        high: int,
        neg_ratio: float = 1.0,
        id: Optional[str] = None,
        seed: Optional[int] = None,
        like: str = 'edge_dst',
        time_key: str = 'edge_time',
    ) -> None:
        super().__init__()
        if not 0 < neg_ratio <= 1:
            raise ValueError(f'neg_ratio must be in (0, 1], got: {neg_ratio}')
        if not low < high:
            raise ValueError(f'low ({low}) must be strictly less than high ({high})')
        self.low, self.high, self.neg_ratio = low, high, neg_ratio
        self._seed = seed
        self._gen: Optional[torch.Generator] = None
        self._rng_seed: Optional[int] = None  # device generator: (seed, call counter, element index)
        self._calls = 0
        # extensions (defaults = the reference's behaviour): draw one negative per element of
        # batch.<like> and copy batch.<time_key>; used to sample for a rank's shard of the batch
        self._like, self._time_key = like, time_key
        self._id = id
        self.__post_init__()
        self._requires |= {like, time_key}

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        n = round(self.neg_ratio * getattr(batch, self._like).size(0))
        device = dg.device
        if n == 0:
            neg = torch.empty((0,), dtype=torch.int32, device=device)
            neg_time = torch.empty((0,), dtype=torch.int64, device=device)
        elif device.type == 'cuda':
            t_in = getattr(batch, self._time_key)
            if t_in.dtype != torch.int64 or not t_in.is_contiguous():
                t_in = t_in.to(torch.int64).contiguous()
            ne = getattr(self, '_new_empty', None)
            if ne is None or ne[0] != device:  # bound new_empty of per-dtype prototypes: cheaper than torch.empty(dtype=, device=)
                ne = self._new_empty = (device, torch.empty(0, dtype=torch.int32, device=device).new_empty,
                                        torch.empty(0, dtype=torch.int64, device=device).new_empty)
            neg = ne[1](n)
            neg_time = ne[2](t_in.shape[0])
            if self._rng_seed is None:
                self._rng_seed = (self._seed if self._seed is not None else torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
            self._calls += 1
            # a rank's share of a sharded batch (like='shard_dst', tgm_amd.dist.EdgeShardHook): its draws are the slice
            # [shard_lo, shard_lo + n) of the ids one rank would draw for the whole batch
            index0 = int(getattr(batch, 'shard_lo', 0) or 0) if self._like != 'edge_dst' else 0
            rc = _native.load().tgmx_random_negatives_at(self.low, self.high, n, self._rng_seed, self._calls, index0, neg.data_ptr(), t_in.data_ptr(),
                                                         t_in.shape[0], neg_time.data_ptr(), _native.stream_ptr(device.index))  # fmt: skip
            if rc:
                _native.check(rc, 'tgmx_random_negatives_at')
        else:
            gen = None
            if self._seed is not None:
                if self._gen is None:
                    self._gen = torch.Generator(device=device)
                    self._gen.manual_seed(self._seed)
                gen = self._gen
            neg = torch.randint(self.low, self.high, (n,), dtype=torch.int32, device=device, generator=gen)
            neg_time = getattr(batch, self._time_key).clone()
        self.add_batch_attribute(batch, 'neg', neg)
        self.add_batch_attribute(batch, 'neg_time', neg_time)
        return batch


_M64 = 0xFFFFFFFFFFFFFFFF
STATUS_BAD_ID, STATUS_OVERFLOW = 1, 2  # tgmx_histneg_t's status bits


def counter_u32(seed: int, stream: int, i: int) -> int:
    """csrc/common.h counter_u32 in Python integers."""
    x = (seed ^ (stream * 0x9E3779B97F4A7C15) ^ (i * 0xD1B54A32D192ED03)) & _M64
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x >> 32


def historical_draw(seed: int, call: int, src: int, n: int) -> int:
    """The rank drawn for source ``src`` with ``n`` >= 1 past events in call ``call``: umulhi32(counter_u32(seed, call, src), n)."""
    return (counter_u32(seed & _M64, call & _M64, src & _M64) * n) >> 32


def pool_words_bound(count: int, num_nodes: int) -> int:
    """Words the segment pool can hold after ``count`` events over ``num_nodes`` ids (derived in csrc/histneg.hip)."""
    return (9 * count + 11 * min(count, num_nodes)) // 4 + 1


@hook
class HistoricalNegativeEdgeSamplerHook(StatefulHook):
    """Sample negative edges from past interactions for dynamic link prediction.

    If a source has no past interaction its negative is ``PADDED_NODE_ID`` (-1) and ``valid_neg_mask`` is False there.  ``seed``
    (extension): the draw's seed, default ``torch.initial_seed()`` read at the first draw.

    Key words: negative sampler, historical, training, link prediction.
    """

    _cls_requires = {'edge_src', 'edge_dst', 'edge_time'}
    _cls_produces = {'neg', 'neg_time', 'valid_neg_mask'}

    def __init__(self, id: Optional[str] = None, seed: Optional[int] = None, _initial_pool_words: int = 1 << 16) -> None:
        super().__init__()
        self._id = id
        self._seed = seed
        self._rng_seed: Optional[int] = None
        self._calls = 0  # never reset: a second epoch draws differently
        self._initial_pool_words = max(1, int(_initial_pool_words))
        self._memory: Optional[torch.Tensor] = None
        self._count: int = 0
        self._hist: Dict[int, List[int]] = {}  # host path: source -> past destinations in arrival order
        self._dev: Optional[dict] = None  # device path: cnt, tail, pool, state, num_nodes
        self._ws: Optional[torch.Tensor] = None
        self._ws_bytes: Dict[int, int] = {}
        self.pool_grown = 0  # host reallocations of the segment pool (tests, tools)
        self.__post_init__()

    def reset_state(self) -> None:
        self._memory = None
        self._count = 0
        self._hist = {}
        self._dev = None

    def check(self) -> None:
        """Raise ``ValueError`` for what the kernels flagged since the last check (one device-to-host read): a source id outside
        ``[0, num_nodes)``, or a segment pool that ran full (its host-side bound makes that a bug, not a condition)."""
        if self._dev is None:
            return
        top, bits = self._dev['state'].tolist()
        if bits:
            self._dev['state'][1:].zero_()
        if bits & STATUS_BAD_ID:
            raise ValueError(f"HistoricalNegativeEdgeSamplerHook: source ids must lie in [0, {self._dev['num_nodes']}); an id outside was offered "
                             '(it drew -1 and joined no history)')  # fmt: skip
        if bits & STATUS_OVERFLOW or top > self._dev['pool'].numel():
            raise ValueError(f"HistoricalNegativeEdgeSamplerHook: the segment pool ran full ({top} of {self._dev['pool'].numel()} words; events were dropped)")

    def histories(self) -> Dict[int, List[int]]:
        """source -> its past destinations in arrival order (device path: read back from the segment chains; for tests and debugging)."""
        if self._dev is None:
            return {s: list(h) for s, h in self._hist.items()}
        cnt, tail, pool = (self._dev[k].cpu().tolist() for k in ('cnt', 'tail', 'pool'))
        out: Dict[int, List[int]] = {}
        for s, n in enumerate(cnt):
            if n == 0:
                continue
            k, off, segs = ((n - 1) // 4 + 1).bit_length() - 1, tail[s], []
            while k >= 0:
                first = 4 * ((1 << k) - 1)
                segs.append(pool[off + 1 : off + 1 + min(4 << k, n - first)])
                off, k = pool[off], k - 1
            out[s] = [d for seg in reversed(segs) for d in seg]
        return out

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        src, dst, time = batch.edge_src, batch.edge_dst, batch.edge_time
        B = int(src.shape[0])
        device = dg.device
        if B == 0:  # (the reference raises from max() of an empty tensor) nothing drawn, nothing appended, the call is not counted
            neg = torch.empty((0,), dtype=torch.int32 if self._count else dst.dtype, device=device)
            neg_time, mask = time.clone(), torch.empty((0,), dtype=torch.bool, device=device)
        else:
            if self._rng_seed is None:
                self._rng_seed = (self._seed if self._seed is not None else torch.initial_seed()) & _M64
            self._calls += 1
            self._grow_memory(B, device)
            step = self._step_device if device.type == 'cuda' else self._step_host
            neg, neg_time, mask = step(dg, src, dst, time, B, device)
            self._count += B
        self.add_batch_attribute(batch, 'neg', neg)
        self.add_batch_attribute(batch, 'neg_time', neg_time)
        self.add_batch_attribute(batch, 'valid_neg_mask', mask)
        return batch

    def _grow_memory(self, B: int, device: torch.device) -> None:
        """The reference's capacity rule (sampler.py:218-233): 2 B at first, then max(2 cap, 2 (count + B)); the tail is zero."""
        if self._memory is None:
            self._memory = torch.zeros((2, 2 * B), dtype=torch.int32, device=device)
        cap = self._memory.size(1)
        if self._count + B > cap:
            grown = torch.zeros((2, max(2 * cap, 2 * (self._count + B))), dtype=torch.int32, device=device)
            grown[:, :cap] = self._memory
            self._memory = grown

    def _step_host(self, dg: DGraph, src, dst, time, B: int, device):
        s_list, d_list = src.tolist(), dst.to(torch.int32).tolist()
        if self._count == 0:
            neg = torch.full((B,), PADDED_NODE_ID, dtype=dst.dtype, device=device)
        else:
            draws = []
            for s in s_list:
                h = self._hist.get(s)
                draws.append(h[historical_draw(self._rng_seed, self._calls, s, len(h))] if h else PADDED_NODE_ID)
            neg = torch.tensor(draws, dtype=torch.int32, device=device)
        for s, d in zip(s_list, d_list):
            self._hist.setdefault(s, []).append(d)
        self._memory[0, self._count : self._count + B] = src
        self._memory[1, self._count : self._count + B] = dst
        return neg, time.clone(), neg != PADDED_NODE_ID

    def _step_device(self, dg: DGraph, src, dst, time, B: int, device):
        lib = _native.load()
        # the graph's node count, a host integer (a view's num_nodes reads its slice's maximum back: only for a graph that is not ours)
        N = getattr(getattr(dg, '_storage', None), 'num_nodes_global', None)
        N = int(dg.num_nodes if N is None else N)
        d = self._dev
        if d is None or d['num_nodes'] < N:
            cnt = torch.zeros(N, dtype=torch.int32, device=device)
            tail = torch.zeros(N, dtype=torch.int32, device=device)
            if d is None:
                d = self._dev = dict(pool=torch.zeros(self._initial_pool_words, dtype=torch.int32, device=device),
                                     state=torch.zeros(2, dtype=torch.int32, device=device))  # fmt: skip
            else:  # a later graph with more nodes: the per-node arrays move, the pool stays
                cnt[: d['num_nodes']] = d['cnt']
                tail[: d['num_nodes']] = d['tail']
            d.update(cnt=cnt, tail=tail, num_nodes=N)
        N = d['num_nodes']
        need = pool_words_bound(self._count + B, N)
        if need > d['pool'].numel():  # sized from the bound alone: pool_top stays on the device
            if need >= 1 << 31:
                raise ValueError(f'HistoricalNegativeEdgeSamplerHook: {self._count + B} events need a pool beyond 2^31 words')
            pool = torch.zeros(min(max(2 * d['pool'].numel(), need), (1 << 31) - 1), dtype=torch.int32, device=device)
            pool[: d['pool'].numel()] = d['pool']  # offsets are pool-relative: they stay valid
            d['pool'] = pool
            self.pool_grown += 1
        dst_dtype = dst.dtype
        if src.dtype not in (torch.int32, torch.int64) or not src.is_contiguous():
            src = src.to(torch.int64).contiguous()
        if dst.dtype not in (torch.int32, torch.int64) or not dst.is_contiguous():
            dst = dst.to(torch.int64).contiguous()
        first = self._count == 0
        if first:  # no history yet: all -1 in edge_dst's dtype as the reference answers, and the kernel draws nothing
            neg = torch.full((B,), PADDED_NODE_ID, dtype=dst_dtype, device=device)
            mask = torch.zeros(B, dtype=torch.bool, device=device)
        else:
            neg = torch.empty(B, dtype=torch.int32, device=device)
            mask = torch.empty(B, dtype=torch.bool, device=device)
        fused_time = time.dtype == torch.int64 and time.is_contiguous()
        neg_time = torch.empty_like(time) if fused_time else time.clone()
        nbytes = self._ws_bytes.get(B)
        if nbytes is None:
            nbytes = self._ws_bytes[B] = int(lib.tgmx_histneg_workspace_bytes(B, N))
            if nbytes == 0:
                raise ValueError(f'HistoricalNegativeEdgeSamplerHook: bad sizes B={B} num_nodes={N}')
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        h = _native.HistNeg(d['cnt'].data_ptr(), d['tail'].data_ptr(), N, d['pool'].data_ptr(), d['pool'].numel(), d['state'].data_ptr(),
                            self._memory.data_ptr(), self._memory.size(1), self._count, self._rng_seed, self._calls)  # fmt: skip
        rc = lib.tgmx_histneg_step(ctypes.byref(h), src.data_ptr(), int(src.dtype == torch.int64), dst.data_ptr(), int(dst.dtype == torch.int64),
                                   time.data_ptr() if fused_time else 0, B, 0 if first else neg.data_ptr(), neg_time.data_ptr() if fused_time else 0,
                                   0 if first else mask.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _native.stream_ptr(device.index))  # fmt: skip
        if rc:
            _native.check(rc, 'tgmx_histneg_step')
        return neg, neg_time, mask
