#!/usr/bin/env python
"""Generate the HistoricalNegativeEdgeSamplerHook fixtures tests/golden/g25_histneg_*.npz by running the REFERENCE.

Runs only where the reference checkout is.  It imports the reference's ``HistoricalNegativeEdgeSamplerHook`` (tgm/hooks/negatives/sampler.py),
drives it on the CPU through a scenario (batches, ``reset_state()`` calls) and records plain .npz data:

    meta            num_nodes (max id + 1), dst_dtype (the dtype the scenario hands edge_dst over in), calls, reset_before (the calls before
                    which reset_state() runs), neg_dtype (per call, the reference's)
    src, dst, ts    the stream (int64), bounds [calls + 1]: call c offers [bounds[c], bounds[c + 1])
    count, mem_cap  [calls] int64: _count and _memory.shape[1] after every call
    mem{c}          [2, count[c]] int32: _memory[:, :_count] after call c
    mask{c}         [B] bool: valid_neg_mask of call c ("the source has a past event")
    adm{c}_off [B + 1], adm{c}_val
                    per position the admissible negatives, i.e. the source's past destinations (arrival order, repeats kept) at that call

The reference's own draws are not recorded (they come from torch's generator); each is checked here to lie in its admissible set, and its
mask to be "the set is not empty" -- with one exception.  The reference matches ``edge_src`` against the WHOLE first row of its log
(``torch.isin(self._memory[0], ...)``), whose unwritten tail is zero: while capacity is left, source id 0 also "has" one event 0 -> 0 per free
column and may draw destination 0 from them, history or none.  That is an artefact of the zero fill, not a semantic anybody asked for (it
depends on the capacity rule); the fixtures record the mask and the sets of the events actually offered, the check below lets the reference's
node-0 answers through where they are such a draw, and the count of those is printed.

    python tests/golden/make_golden_histneg.py

  g25_histneg_unit_stream    the 12-edge stream of the reference's test_hst_sampling, batch 4
  g25_histneg_hub_crossing   one source accumulates 29 events over eight calls, crossing ranks 4, 12 and 28 (the segment boundaries)
  g25_histneg_hub_one_batch  one batch offers 30 events of a new source among singletons
  g25_histneg_mixed          repeated sources, never-seen sources and sources seen only as destinations
  g25_histneg_extreme_ids    sources 0 and num_nodes - 1
  g25_histneg_first_int64    edge_dst handed over as int64 (the first call answers in that dtype)
  g25_histneg_wiki_small     2 000 events of tgm_amd.synth.make_stream in batches of 200
  g25_histneg_reset          reset_state() mid-stream, then two more batches
"""
from __future__ import annotations

import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_pyg_stub'))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tgm.hooks.negatives.sampler import HistoricalNegativeEdgeSamplerHook  # noqa: E402

from tgm_amd.synth import make_stream  # noqa: E402

TORCH = {'int64': torch.int64, 'int32': torch.int32}


def scenario(name: str, calls, dst_dtype: str = 'int32', reset_before=()) -> None:
    """calls: [(src, dst, ts)]"""
    hook = HistoricalNegativeEdgeSamplerHook()
    dg = types.SimpleNamespace(device=torch.device('cpu'))
    past: dict = {}
    arrays, counts, caps, neg_dtypes, phantom = {}, [], [], [], 0
    torch.manual_seed(2500)
    for c, (s, d, t) in enumerate(calls):
        s, d, t = (np.asarray(v, dtype=np.int64) for v in (s, d, t))
        if c in reset_before:
            hook.reset_state()
            past = {}
        batch = types.SimpleNamespace(edge_src=torch.tensor(s).to(torch.int32), edge_dst=torch.tensor(d).to(TORCH[dst_dtype]), edge_time=torch.tensor(t))
        hook(dg, batch)
        adm = [past.get(int(v), []) for v in s]
        neg, ref_mask = batch.neg.numpy(), batch.valid_neg_mask.numpy()
        mask = np.array([len(a) > 0 for a in adm])
        # node 0 apart (see above): the reference may also answer 0 there, drawn from the unwritten tail of its log
        tail_hit = (s == 0) & (neg == 0) & (c > 0)
        phantom += int((tail_hit & ~np.array([0 in a for a in adm])).sum())
        assert np.array_equal(ref_mask[~tail_hit], mask[~tail_hit]), (name, c, 'mask')
        assert all(hit or ((n in a) if a else n == -1) for n, a, hit in zip(neg.tolist(), adm, tail_hit)), (name, c, 'draw outside its set')
        assert all(neg[i] == neg[j] for i in range(len(s)) for j in range(i) if s[i] == s[j]), (name, c, 'duplicates')
        assert torch.equal(batch.neg_time, batch.edge_time)
        for a, b in zip(s.tolist(), d.tolist()):
            past.setdefault(a, []).append(b)
        past = {k: list(v) for k, v in past.items()}
        counts.append(hook._count)
        caps.append(hook._memory.shape[1])
        neg_dtypes.append(str(batch.neg.dtype)[6:])
        assert hook._memory.dtype == torch.int32 and not hook._memory[:, hook._count :].any()
        arrays[f'mem{c}'] = hook._memory[:, : hook._count].numpy().copy()
        arrays[f'mask{c}'] = mask
        arrays[f'adm{c}_off'] = np.cumsum([0] + [len(a) for a in adm]).astype(np.int64)
        arrays[f'adm{c}_val'] = np.array([x for a in adm for x in a], dtype=np.int64)
    cat = lambda i: np.concatenate([np.asarray(call[i], dtype=np.int64) for call in calls])
    bounds = np.cumsum([0] + [len(call[0]) for call in calls]).astype(np.int64)
    meta = dict(num_nodes=int(max(cat(0).max(), cat(1).max())) + 1, dst_dtype=dst_dtype, calls=len(calls), reset_before=list(reset_before),
                neg_dtype=neg_dtypes)
    path = os.path.join(HERE, f'g25_histneg_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), src=cat(0), dst=cat(1), ts=cat(2), bounds=bounds,
                        count=np.array(counts, dtype=np.int64), mem_cap=np.array(caps, dtype=np.int64), **arrays)
    size = os.path.getsize(path)
    assert size < 200_000, (name, size)
    print(f'g25_histneg_{name}: {size} bytes, {len(calls)} calls, counts {counts}, caps {caps}, valid {[int(arrays[f"mask{c}"].sum()) for c in range(len(calls))]}, node-0 draws from the unwritten tail {phantom}')


def split(src, dst, sizes):
    calls, lo = [], 0
    for n in sizes:
        calls.append((src[lo : lo + n], dst[lo : lo + n], np.arange(lo, lo + n)))
        lo += n
    assert lo == len(src)
    return calls


def unit_stream() -> None:
    e = [[1, 5], [7, 6], [2, 8], [7, 8], [1, 7], [9, 10], [3, 10], [1, 9], [3, 11], [2, 10], [7, 2], [3, 5]]
    scenario('unit_stream', split([a for a, _ in e], [b for _, b in e], [4, 4, 4]))


def hub_crossing() -> None:
    rng = np.random.default_rng(2501)
    hub, per_call = 5, [3, 2, 4, 4, 5, 6, 5, 3]  # cumulative 3, 5, 9, 13, 18, 24, 29: past 4 in call 1, 12 in call 3, 28 in call 6; call 7 draws from 29+
    assert sum(per_call[:7]) == 29
    calls, t0, nxt = [], 0, 100
    for k in per_call:
        others = rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11], 8 - k)
        s = np.concatenate([np.full(k, hub), others])
        s = s[rng.permutation(8)]
        d = np.arange(nxt, nxt + 8)  # every destination distinct, so a draw names its rank
        nxt += 8
        calls.append((s, d, np.arange(t0, t0 + 8)))
        t0 += 8
    scenario('hub_crossing', calls)


def hub_one_batch() -> None:
    rng = np.random.default_rng(2502)
    s0 = np.concatenate([np.full(30, 7), np.arange(20, 30)])[rng.permutation(40)]
    d0 = np.arange(200, 240)
    s1 = np.array([7, 20, 7, 31, 29, 7, 25, 0])
    s2 = np.array([7, 7, 31, 0, 24, 7])
    calls = [(s0, d0, np.arange(40)), (s1, np.arange(300, 308), np.arange(40, 48)), (s2, np.arange(400, 406), np.arange(48, 54))]
    scenario('hub_one_batch', calls)


def mixed() -> None:
    rng = np.random.default_rng(2503)
    calls, t0 = [], 0
    for c in range(6):
        n = int(rng.integers(5, 30))
        hi = 12 if c < 3 else 20  # ids 12..19: destinations only during the first three calls, sources after
        s = rng.integers(0, hi, n)
        d = rng.integers(8, 20, n)
        calls.append((s, d, np.sort(rng.integers(t0, t0 + 50, n))))
        t0 += 50
    scenario('mixed', calls)


def extreme_ids() -> None:
    s = [0, 49, 0, 3, 49, 0, 49, 49, 0, 3, 0, 49]
    d = [49, 0, 1, 49, 48, 0, 49, 2, 3, 0, 48, 1]
    scenario('extreme_ids', split(s, d, [3, 3, 3, 3]))


def first_int64() -> None:
    rng = np.random.default_rng(2504)
    s, d = rng.integers(0, 6, 18), rng.integers(0, 9, 18)
    scenario('first_int64', split(s, d, [6, 6, 6]), dst_dtype='int64')


def wiki_small() -> None:
    st = make_stream('wiki', seed=2505, num_edges=2000, n_src=60, n_dst=40, edge_dim=0)
    src, dst, ts = st.src.numpy().astype(np.int64), st.dst.numpy().astype(np.int64), st.ts.numpy()
    scenario('wiki_small', [(src[a : a + 200], dst[a : a + 200], ts[a : a + 200]) for a in range(0, 2000, 200)])


def reset() -> None:
    rng = np.random.default_rng(2506)
    s, d = rng.integers(0, 7, 50), rng.integers(0, 15, 50)
    scenario('reset', split(s, d, [10, 10, 10, 12, 8]), reset_before=(3,))


if __name__ == '__main__':
    torch.set_num_threads(1)
    unit_stream()
    hub_crossing()
    hub_one_batch()
    mixed()
    extreme_ids()
    first_int64()
    wiki_small()
    reset()
