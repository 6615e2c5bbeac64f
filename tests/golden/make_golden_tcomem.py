#!/usr/bin/env python
"""Generate the tCoMemPredictor and PopTrackPredictor fixtures tests/golden/g20_tcomem_*.npz, g21_poptrack_*.npz by running the REFERENCE.

Runs only where the reference checkout is.  It imports the reference's ``tCoMemPredictor`` (tgm/nn/modules/t_comem.py) and
``PopTrackPredictor`` (tgm/nn/modules/poptrack.py), drives them on the CPU through a scenario (the constructor, then ``update`` calls) and
records plain .npz data.  g20:

    meta            num_nodes, k, co_occurrence_weight, window_ratio, stream_dtype (the dtype the scenario hands the stream over in), and per
                    call the list of its queries as {dtype, rows}; rows > 0: the query is `rows`-long runs of one source, its destination
                    first and its negatives after it (the evaluation loop's one-against-many form)
    src, dst, ts    the stream (int64), bounds [calls + 1]: call c offers [bounds[c], bounds[c + 1]); call 0 is the constructor
    window_start [calls] float64, window_end [calls] int64, window_size [calls] int64, after every call
    ring_ts [N, calls, k] float32, ring_dst [N, calls, k] int64, len, pos, pop [calls, N] float32
                    the reference's state tensors after every call ([:, c] of the first two is its recent_ts / recent_dst after call c;
                    a node's rows lie next to each other over the calls because they change little, which the compression needs)
    co{c}_pairs [n, 2], co{c}_count [n]   its pair counts after call c, one row per unordered pair (smaller id first), sorted; asserted
                    here: both directions of the reference's nested dict hold that count
    q{c}_{j}_src, q{c}_{j}_dst (int64), q{c}_{j}_pred (float32, the reference's answer), q{c}_{j}_pred64 (float64: the restatement's
                    float64 evaluation of the same state)

and g20_tcomem_self_noise.json: per fixture the reference's own float32 distance from the float64 record, max |a - b| / max(1, |b|).

    python tests/golden/make_golden_tcomem.py

Every scenario is also run through tests/tcomem_restate.py: state and window must agree bit for bit, the float32 scores to 1e-6.

  g20_tcomem_ring_wrap_k2, _counts, _popularity, _no_history, _window_moves
                    the situations the reference's unit tests exercise through the public surface, with their float32 tensors
  g20_tcomem_wiki_small_k{50,5}_{int64,float32}
                    2 000 events over 60 x 40 nodes, 1 000 in the constructor, five batches of 200, each positive of the NEXT batch queried
                    with 49 negatives
  g20_tcomem_epoch_f32
                    timestamps near 1.6e9: asserted here that exact arithmetic would store and mask differently
  g20_tcomem_burst  more than k events of one source inside one call and across calls
  g20_tcomem_selfloop_bothways, _equal_ts
  g20_tcomem_stale  a late event with an old timestamp, then a jump of `end` that cuts most ring entries (asserted: some cut, some kept)
  g20_tcomem_query_dtypes
                    int32 / int64 / float32 / float64 queries on one state
  g21_poptrack_d09, _d10, _d037, _int32
                    ten updates with repeated destinations inside a call; popularity after every call and a query of every node
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_pyg_stub'))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tgm.nn.modules.poptrack import PopTrackPredictor  # noqa: E402
from tgm.nn.modules.t_comem import tCoMemPredictor  # noqa: E402

import tcomem_restate as tr  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

TORCH = {'int64': torch.int64, 'int32': torch.int32, 'float32': torch.float32, 'float64': torch.float64}
NOISE = {}


def scenario(name: str, num_nodes: int, k: int, weight: float, calls, queries, stream_dtype: str = 'int64', after_call=None,
             exact_must_differ: bool = False) -> None:  # fmt: skip
    """calls: [(src, dst, ts)] (call 0 is the constructor); queries[c]: [(src, dst, dtype, rows)] asked after call c"""
    td = TORCH[stream_dtype]
    as_t = lambda v: torch.tensor(np.asarray(v, dtype=np.int64)).to(td)
    arrays, state, meta_q, starts, ends, sizes = {}, {}, [], [], [], []
    ref = ours = exact = None
    diff_stored = diff_mask = False
    noise = 0.0
    for c, (s, d, t) in enumerate(calls):
        if c == 0:
            ref = tCoMemPredictor(as_t(s), as_t(d), as_t(t), num_nodes, k, 0.15, weight)
            ours = tr.TCoMemRestated(s, d, t, num_nodes, k, weight)
            exact = tr.TCoMemRestated(s, d, t, num_nodes, k, weight, arithmetic='exact')
        else:
            ref.update(as_t(s), as_t(d), as_t(t))
            ours.update(s, d, t)
            exact.update(s, d, t)
        starts.append(float(ref.window_start))
        ends.append(int(ref.window_end))
        sizes.append(int(ref.window_size))
        assert (ours.window_start, ours.window_end, ours.window_size) == (starts[-1], ends[-1], sizes[-1]), (name, c, 'window')
        assert ref.recent_ts.dtype == torch.float32 and ref.recent_dst.dtype == torch.int64
        for mine, theirs, what in ((ours.recent_ts, ref.recent_ts, 'ts'), (ours.recent_dst, ref.recent_dst, 'dst'), (ours.len, ref.recent_len, 'len'),
                                   (ours.pos, ref.recent_pos, 'pos'), (ours.pop, ref.popularity, 'pop')):  # fmt: skip
            assert np.array_equal(mine.astype(theirs.numpy().dtype), theirs.numpy()), (name, c, what)
            state.setdefault(what, []).append(theirs.numpy().copy())
        nested = {int(a): {int(b): int(v) for b, v in row.items()} for a, row in ref.node_to_co_occurrence.items() if row}
        assert nested == ours.nested_counts(), (name, c, 'counts')
        arrays[f'co{c}_pairs'], arrays[f'co{c}_count'] = ours.count_arrays()
        diff_stored |= not np.array_equal(exact.recent_ts, ours.recent_ts.astype(np.float64))
        diff_mask |= any(not np.array_equal(exact._mask(v), ours._mask(v)) for v in range(num_nodes))
        if after_call:
            after_call(c, ours)
        meta_q.append([])
        for j, (qs, qd, dtype, rows) in enumerate(queries[c]):
            qs, qd = np.asarray(qs, dtype=np.int64), np.asarray(qd, dtype=np.int64)
            pred = ref(torch.tensor(qs).to(TORCH[dtype]), torch.tensor(qd).to(TORCH[dtype]))
            assert pred.dtype == torch.float32 and pred.shape == (len(qs),)
            pred, mine, pred64 = pred.numpy(), ours.scores(qs, qd, dtype), ours.scores64(qs, qd, dtype)
            assert tr.rel_err(mine, pred) < 1e-6, (name, c, j, tr.rel_err(mine, pred))
            if dtype in tr.INTEGER_QUERIES:  # the truncated term: the answer is the base score alone, whatever the pair
                assert all(len(set(pred[qs == v].tolist())) == 1 for v in set(qs.tolist())), (name, c, j, 'integer queries')
            noise = max(noise, tr.rel_err(pred, pred64))
            arrays[f'q{c}_{j}_src'], arrays[f'q{c}_{j}_dst'], arrays[f'q{c}_{j}_pred'], arrays[f'q{c}_{j}_pred64'] = qs, qd, pred, pred64
            meta_q[-1].append(dict(dtype=dtype, rows=rows))
    if exact_must_differ:
        assert diff_stored and diff_mask, f'{name}: exact arithmetic is indistinguishable here (stored {diff_stored}, mask {diff_mask})'
    cat = lambda i: np.concatenate([np.asarray(call[i], dtype=np.int64) for call in calls])
    bounds = np.cumsum([0] + [len(call[0]) for call in calls]).astype(np.int64)
    meta = dict(num_nodes=num_nodes, k=k, co_occurrence_weight=weight, window_ratio=0.15, stream_dtype=stream_dtype, calls=len(calls), queries=meta_q)
    arrays.update(ring_ts=np.stack(state['ts'], 1), ring_dst=np.stack(state['dst'], 1), len=np.stack(state['len']), pos=np.stack(state['pos']),
                  pop=np.stack(state['pop']))  # fmt: skip
    path = os.path.join(HERE, f'g20_tcomem_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), src=cat(0), dst=cat(1), ts=cat(2), bounds=bounds,
                        window_start=np.array(starts, dtype=np.float64), window_end=np.array(ends, dtype=np.int64),
                        window_size=np.array(sizes, dtype=np.int64), **arrays)  # fmt: skip
    size = os.path.getsize(path)
    assert size < 200_000, (name, size)
    NOISE[f'g20_tcomem_{name}'] = noise
    print(f'g20_tcomem_{name}: {size} bytes, {len(calls)} calls, self-noise {noise:.3e}')


def q(pairs, dtype='float32'):
    return ([p[0] for p in pairs], [p[1] for p in pairs], dtype, 0)


EVERYONE = [(1, 2), (2, 1), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (1, 1), (1, 3), (1, 4), (9, 1), (2, 9), (4, 4)]


def unit_test_situations() -> None:
    ask = lambda calls: [[q(EVERYONE)]] * len(calls)
    calls = [([1, 1, 1], [2, 3, 4], [1, 2, 3])]
    scenario('ring_wrap_k2', 10, 2, 0.8, calls, ask(calls), 'float32')
    calls = [([1, 1], [2, 2], [1, 2]), ([1], [2], [3]), ([1, 1, 1], [2, 2, 2], [4, 5, 6])]
    scenario('counts', 10, 5, 1.0, calls, ask(calls), 'float32')
    calls = [([1, 2, 3], [4, 4, 4], [1, 2, 3])]
    scenario('popularity', 10, 5, 0.8, calls, ask(calls), 'float32')
    calls = [([1], [2], [1])]
    scenario('no_history', 10, 5, 0.8, calls, ask(calls), 'float32')
    calls = [([1, 2, 3, 4, 5, 6], [2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6]), ([3], [4], [5]), ([7], [8], [7]), ([8], [9], [11])]
    scenario('window_moves', 10, 5, 0.8, calls, ask(calls), 'float32')


def wiki_small(k: int, dtype: str) -> None:
    s = make_stream('wiki', seed=1900, num_edges=2000, n_src=60, n_dst=40, edge_dim=0)
    src, dst, ts = s.src.numpy().astype(np.int64), s.dst.numpy().astype(np.int64), s.ts.numpy()
    bounds = [0, 1000, 1200, 1400, 1600, 1800, 2000]
    calls = [(src[a:b], dst[a:b], ts[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    rng = np.random.default_rng(2000)
    queries = []
    for c in range(len(calls)):
        if c + 2 >= len(bounds):  # no next batch
            queries.append([])
            continue
        a, b = bounds[c + 1], bounds[c + 2]
        neg = rng.integers(60, 100, (b - a, 49))
        queries.append([(np.repeat(src[a:b], 50), np.concatenate([dst[a:b, None], neg], 1).reshape(-1), dtype, 50)])
    scenario(f'wiki_small_k{k}_{dtype}', 100, k, 0.8, calls, queries)


def epoch_f32() -> None:
    rng = np.random.default_rng(2002)
    base = 1_600_000_000
    assert tr.TCoMemRestated([0, 1], [1, 2], [base, base + 1000], 3, 2).window_start == base  # the issue's figures
    calls, lo = [], 0
    for n, span in ((100, 1000), (20, 100), (30, 300), (30, 300)):  # few events a source: the rings (k = 8) keep entries near the window start
        t = np.sort(rng.integers(lo, lo + span + 1, n))
        t[0], t[-1] = lo, lo + span
        if not calls:
            t[1:5] = [70, 80, 90, 95]  # below the exact start after call 1 (100), at the float32 one (128) once rounded
            t = np.sort(t)
        calls.append((rng.integers(0, 20, n), rng.integers(20, 35, n), base + t))
        lo += span
    pairs = [(a, b) for a in range(20) for b in (20, 27, 34)]
    scenario('epoch_f32', 35, 8, 0.8, calls, [[q(pairs, 'int64'), q(pairs, 'float32')]] * len(calls), exact_must_differ=True)


def burst() -> None:
    pairs = [(a, b) for a in range(4) for b in range(4, 8)]
    calls = [([0, 1, 0, 0, 0, 2, 0, 0, 0], [4, 5, 5, 6, 7, 4, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7, 8, 9]),  # seven of source 0, k = 3
             ([0, 0, 1, 0, 0, 0], [7, 6, 4, 5, 4, 7], [10, 11, 12, 13, 14, 15]),                      # five more in one update
             ([0, 1], [6, 6], [16, 17]),                                                               # across calls: one at a time
             ([0], [5], [18]), ([3, 0], [4, 4], [19, 20])]
    scenario('burst', 8, 3, 0.8, calls, [[q(pairs, 'int64'), q(pairs, 'float32')]] * len(calls))
    # the issue's figure: five events of one source with k = 3
    five = tr.TCoMemRestated([0] * 5, [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], 6, 3)
    assert five.recent_ts[0].tolist() == [4, 5, 3] and five.recent_dst[0].tolist() == [4, 5, 3], (five.recent_ts[0], five.recent_dst[0])


def selfloop_bothways() -> None:
    pairs = [(a, b) for a in range(1, 4) for b in range(1, 4)]
    calls = [([1, 1, 2, 2, 1], [1, 2, 1, 2, 1], [1, 2, 3, 4, 5]), ([2, 3, 3], [1, 3, 1], [6, 7, 8])]
    scenario('selfloop_bothways', 5, 4, 0.8, calls, [[q(pairs, 'float32'), q(pairs, 'float64'), q(pairs, 'int64')]] * len(calls))


def equal_ts() -> None:
    pairs = [(a, b) for a in range(4) for b in range(4, 7)]
    calls = [([0, 1, 2, 0], [4, 5, 6, 5], [50, 50, 50, 50]), ([1, 3], [4, 6], [50, 51]), ([2], [4], [55])]
    scenario('equal_ts', 7, 3, 0.8, calls, [[q(pairs, 'float32'), q(pairs, 'int64')]] * len(calls))


def stale() -> None:
    rng = np.random.default_rng(2003)
    seen = []

    def filled_and_kept(c, model):
        filled = int(sum(model.len))
        kept = int(sum(model._mask(v).sum() for v in range(model.N)))
        seen.append((filled, kept))

    calls = [(rng.integers(0, 5, 40), rng.integers(5, 10, 40), np.sort(rng.integers(0, 1001, 40))),
             ([1, 2], [6, 7], [5, 990]),                                                   # a late event with an old timestamp
             (rng.integers(0, 5, 6), rng.integers(5, 10, 6), [5200, 5400, 300, 5900, 6000, 5950])]  # the jump
    calls[0][2][0], calls[0][2][-1] = 0, 1000
    pairs = [(a, b) for a in range(5) for b in range(5, 10)]
    scenario('stale', 10, 8, 0.8, calls, [[q(pairs, 'int64'), q(pairs, 'float32')]] * len(calls), after_call=filled_and_kept)
    filled, kept = seen[-1]
    assert filled >= 35 and 0 < kept < filled // 2, seen  # k = 8 over 5 sources: the rings are all but full; the jump cuts most entries, not all
    print(f'  stale: after the jump {filled - kept} of {filled} filled entries are cut')


def query_dtypes() -> None:
    rng = np.random.default_rng(2004)
    calls = [(rng.integers(0, 12, 60), rng.integers(0, 12, 60), np.sort(rng.integers(0, 500, 60))) for _ in range(2)]
    pairs = [(a, b) for a in range(12) for b in range(12)]
    scenario('query_dtypes', 12, 6, 0.7, calls, [[q(pairs, 'int64'), q(pairs, 'int32'), q(pairs, 'float32'), q(pairs, 'float64')]] * 2)


def poptrack(name: str, decay: float, stream_dtype: str = 'int64') -> None:
    rng = np.random.default_rng(2100)
    N = 30
    td = TORCH[stream_dtype]
    as_t = lambda v: torch.tensor(np.asarray(v, dtype=np.int64)).to(td)
    calls = [(rng.integers(0, N, n), rng.integers(0, 12, n) if c % 2 else rng.integers(0, N, n), np.sort(rng.integers(10 * c, 10 * c + 10, n)))
             for c, n in enumerate((50, 1, 7, 64, 65, 20, 3, 100, 20, 20, 33))]  # the constructor and ten updates; destinations repeat
    arrays, repeats = {}, 0
    qd = np.arange(N, dtype=np.int64)
    for c, (s, d, t) in enumerate(calls):
        repeats += len(set(d.tolist())) < len(d)
        if c == 0:
            ref, ours = PopTrackPredictor(as_t(s), as_t(d), as_t(t), N, 5, decay), tr.PopTrackRestated(s, d, t, N, 5, decay)
        else:
            ref.update(as_t(s), as_t(d), as_t(t))
            ours.update(s, d, t)
        assert ref.popularity.dtype == torch.float32 and np.array_equal(ref.popularity.numpy(), ours.popularity), (name, c)  # bit for bit
        pred = ref(as_t(qd), as_t(qd[::-1].copy()))
        assert pred.dtype == torch.float32 and np.array_equal(pred.numpy(), ours(qd, qd[::-1]))
        arrays[f'pop{c}'], arrays[f'q{c}_pred'] = ref.popularity.numpy().copy(), pred.numpy()
    assert repeats >= 7, repeats  # destinations repeat inside most calls
    try:
        ref(torch.tensor([1.0]), torch.tensor([1.0]))
        raise AssertionError('float ids were accepted')
    except IndexError:
        pass
    cat = lambda i: np.concatenate([np.asarray(call[i], dtype=np.int64) for call in calls])
    bounds = np.cumsum([0] + [len(call[0]) for call in calls]).astype(np.int64)
    meta = dict(num_nodes=N, k=5, decay=decay, stream_dtype=stream_dtype, calls=len(calls))
    path = os.path.join(HERE, f'g21_poptrack_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), src=cat(0), dst=cat(1), ts=cat(2), bounds=bounds,
                        q_src=qd, q_dst=qd[::-1].copy(), **arrays)  # fmt: skip
    print(f'g21_poptrack_{name}: {os.path.getsize(path)} bytes, {len(calls)} calls')


if __name__ == '__main__':
    torch.set_num_threads(1)
    unit_test_situations()
    for k in (50, 5):
        for dtype in ('int64', 'float32'):
            wiki_small(k, dtype)
    epoch_f32()
    burst()
    selfloop_bothways()
    equal_ts()
    stale()
    query_dtypes()
    with open(os.path.join(HERE, 'g20_tcomem_self_noise.json'), 'w') as f:
        json.dump(NOISE, f, indent=1, sort_keys=True)
        f.write('\n')
    poptrack('d09', 0.9)
    poptrack('d10', 1.0)
    poptrack('d037', 0.37)
    poptrack('int32', 0.9, 'int32')
