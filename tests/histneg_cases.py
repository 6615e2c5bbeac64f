"""Shared by tests/test_histneg_cpu.py and tests/test_histneg_gpu.py: the g25 fixtures as call lists, the assertions a replay makes against
them, and the streams both files run.  ``replay`` drives one HistoricalNegativeEdgeSamplerHook over a fixture's calls on whatever device the
graph is on."""
from __future__ import annotations

import glob
import os
import types

import numpy as np
import torch

import golden_util
from tgm_amd import DGData, DGraph
from tgm_amd.hooks import HistoricalNegativeEdgeSamplerHook
from tgm_amd.hooks.negatives import historical_draw  # noqa: F401  (the tests restate draws with it)

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_util.GOLDEN_DIR, 'g25_histneg_*.npz')))
EXPECTED = ['unit_stream', 'hub_crossing', 'hub_one_batch', 'mixed', 'extreme_ids', 'first_int64', 'wiki_small', 'reset']
TORCH = {'int64': torch.int64, 'int32': torch.int32}


def graph(src, dst, ts, device='cpu') -> DGraph:
    """A graph over the whole stream: the hook reads its device and its node count."""
    order = np.argsort(np.asarray(ts), kind='stable')
    ei = torch.tensor(np.stack([np.asarray(src)[order], np.asarray(dst)[order]], 1).astype(np.int32))
    return DGraph(DGData.from_raw(torch.tensor(np.asarray(ts)[order].astype(np.int64)), ei), device=device)


def batch_of(src, dst, ts, device, dst_dtype=torch.int32):
    T = lambda v, dt: torch.tensor(np.asarray(v, dtype=np.int64)).to(dt).to(device)
    return types.SimpleNamespace(edge_src=T(src, torch.int32), edge_dst=T(dst, dst_dtype), edge_time=T(ts, torch.int64))


def fixture_calls(name: str):
    """-> meta, arrays, [(src, dst, ts)] per call"""
    meta, a = golden_util.load(name)
    b = a['bounds']
    return meta, a, [(a['src'][b[c] : b[c + 1]], a['dst'][b[c] : b[c + 1]], a['ts'][b[c] : b[c + 1]]) for c in range(meta['calls'])]


def replay(name: str, device: str, **hook_kw):
    """Run the fixture on `device`, assert everything it records, return per call (neg, mask, memory, count) on the host."""
    meta, a, calls = fixture_calls(name)
    dg = graph(a['src'], a['dst'], a['ts'], device)
    assert dg._storage.num_nodes_global == meta['num_nodes']
    hook = HistoricalNegativeEdgeSamplerHook(**hook_kw)
    out = []
    for c, (s, d, t) in enumerate(calls):
        if c in meta['reset_before']:
            hook.reset_state()
            assert hook._memory is None and hook._count == 0
        batch = batch_of(s, d, t, dg.device, TORCH[meta['dst_dtype']])
        assert hook(dg, batch) is batch
        neg, mask = batch.neg.cpu(), batch.valid_neg_mask.cpu()
        where = f'{name} call {c}'
        assert hook._count == a['count'][c] and type(hook._count) is int, where
        assert tuple(hook._memory.shape) == (2, a['mem_cap'][c]) and hook._memory.dtype == torch.int32, where
        mem = hook._memory.cpu().numpy()
        assert np.array_equal(mem[:, : hook._count], a[f'mem{c}']) and not mem[:, hook._count :].any(), where
        assert str(neg.dtype)[6:] == meta['neg_dtype'][c], where  # int32 once history exists, edge_dst's dtype on the first call
        assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), a[f'mask{c}']), where
        assert torch.equal(mask, neg != -1), where
        off, val = a[f'adm{c}_off'], a[f'adm{c}_val']
        for i, n in enumerate(neg.tolist()):
            allowed = val[off[i] : off[i + 1]]
            assert (n in allowed) if len(allowed) else n == -1, f'{where} position {i}: {n} not among {allowed.tolist()}'
        for i in range(len(s)):  # every position of one source gets one negative
            assert neg[i] == neg[int(np.flatnonzero(s == s[i])[0])], where
        assert torch.equal(batch.neg_time.cpu(), torch.tensor(t)) and batch.neg_time.data_ptr() != batch.edge_time.data_ptr(), where
        out.append((neg, mask, mem.copy(), hook._count))
    return hook, out


# ---- streams beyond the fixtures (device against host, bit for bit) ----------------------------------------------------------------------


def extra_streams():
    """name -> (calls, hook keywords).  Destinations are distinct within a stream wherever a test wants a draw to name its rank."""
    rng = np.random.default_rng(2510)
    streams = {}
    # a source taken from 0 to 29 events one per call, then drawn once (test_every_rank_is_drawn repeats it over seeds until all 29 ranks came back)
    streams['one_per_call'] = ([([4], [100 + c], [c]) for c in range(29)] + [([4, 2], [900, 5], [29, 29])], {})
    streams['skewed_256'] = ([(np.full(256, 3), np.arange(1000, 1256), np.arange(256)), ([3, 1, 3], [7, 8, 9], [256, 257, 258]),
                              (np.full(256, 3), np.arange(2000, 2256), np.arange(259, 515)), ([3], [1], [600])], {})  # fmt: skip
    streams['all_distinct'] = ([(np.arange(300), rng.integers(0, 300, 300), np.arange(300)), (rng.permutation(300), rng.integers(0, 300, 300), np.arange(300, 600)),
                                (rng.permutation(300), rng.integers(0, 300, 300), np.arange(600, 900))], {})  # fmt: skip
    streams['batch_of_one'] = ([([int(rng.integers(0, 3))], [int(rng.integers(0, 50))], [c]) for c in range(40)], {})
    streams['one_node'] = ([(np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.arange(n)) for n in (1, 5, 1, 40, 3)], {})
    # long enough for the pool (from 8 words) and the log to be reallocated by the host more than twice
    long = [(rng.integers(0, 40, 64), rng.integers(0, 500, 64), np.arange(c * 64, (c + 1) * 64)) for c in range(24)]
    streams['reallocating'] = (long, dict(_initial_pool_words=8))
    return streams


def stream_graph(calls, device: str) -> DGraph:
    return graph(*(np.concatenate([np.asarray(c[i], dtype=np.int64) for c in calls]) for i in range(3)), device)


def run_stream(calls, device: str, seed: int = 7, dg=None, **hook_kw):
    dg = dg if dg is not None else stream_graph(calls, device)
    hook = HistoricalNegativeEdgeSamplerHook(seed=seed, **hook_kw)
    out = []
    for s, d, t in calls:
        batch = hook(dg, batch_of(s, d, t, dg.device))
        out.append((batch.neg.cpu(), batch.valid_neg_mask.cpu(), hook._memory.cpu().clone(), hook._count))
    return hook, out


def assert_same_runs(a, b, what: str) -> None:
    assert len(a) == len(b)
    for c, ((n0, m0, mem0, c0), (n1, m1, mem1, c1)) in enumerate(zip(a, b)):
        assert n0.dtype == n1.dtype and torch.equal(n0, n1), f'{what} call {c}: neg'
        assert torch.equal(m0, m1), f'{what} call {c}: mask'
        assert torch.equal(torch.as_tensor(mem0), torch.as_tensor(mem1)) and c0 == c1, f'{what} call {c}: memory'
