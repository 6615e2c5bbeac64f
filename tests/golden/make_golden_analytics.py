#!/usr/bin/env python
"""Generate the fixtures of the analytics and seen-node hooks by running the REFERENCE:

    tests/golden/g27_batch_analytics_*.npz   BatchAnalyticsHook            (tgm/hooks/analytics/batch_analytics.py)
    tests/golden/g28_seen_nodes_*.npz        EdgeEventsSeenNodesTrackHook  (tgm/hooks/node_tracks.py)
    tests/golden/g29_node_analytics_*.npz    NodeAnalyticsHook             (tgm/hooks/analytics/node_analytics.py)

Runs only where the reference checkout is.  It imports the reference's three classes in place, drives them on the CPU through a scenario --
a list of steps, each 'reset' or a batch given as a dict of arrays (a missing field is None) -- and records plain data:

    meta          steps ('reset' or the call's number), the constructor's arguments, dict key orders, per-call scalars
    {field}, {field}_len, meta['dtypes'][field]
                  the inputs: every call's vector end to end (widened to int64), its length per call (-1: the field is None) and the dtype
                  the scenario hands it over in
    g27           meta['out'][i]: the seven statistics of call i, as Python numbers
    g28           seen_nodes, batch_nodes_mask: packed like the inputs; mask: _seen_mask after the last call; meta['marked'][i]: its sum after call i
    g29           ids (packed): node_stats' keys in order; stats [sum K, 6] float64: their values in meta['node_keys'] order; macro [calls, 2],
                  edge [calls, 3] in meta['macro_keys'] / meta['edge_keys'] order (every integer here is exact in float64); meta['suffixed'][i]:
                  whether the three were written with the id suffix; meta['sizes'][i]: distinct times, pairs, (node, neighbour) and
                  (node, time) entries after call i

The behaviours the hooks' docstrings call "kept" are asserted here against the reference itself: if it does not behave that way this fails.

    python tests/golden/make_golden_analytics.py
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
from tgm.hooks.analytics.batch_analytics import BatchAnalyticsHook  # noqa: E402
from tgm.hooks.analytics.node_analytics import NodeAnalyticsHook  # noqa: E402
from tgm.hooks.node_tracks import EdgeEventsSeenNodesTrackHook  # noqa: E402

from tgm_amd.synth import make_stream  # noqa: E402

FIELDS = ('edge_src', 'edge_dst', 'edge_time', 'node_x_nids', 'node_x_time', 'node_y_nids')
BA_KEYS = ('num_edge_events', 'num_node_events', 'num_unique_timestamps', 'num_unique_nodes', 'avg_degree', 'num_repeated_edge_events',
           'num_repeated_node_events')  # fmt: skip
DG = types.SimpleNamespace(device=torch.device('cpu'))
I32, I64 = np.int32, np.int64


def B(src=None, dst=None, t=None, nids=None, nt=None, y=None, ids=I32, times=I64):
    """One batch; ids / times: the dtypes the id and time fields are handed over in."""
    conv = lambda v, dt: None if v is None else np.asarray(v, dtype=dt)
    return dict(edge_src=conv(src, ids), edge_dst=conv(dst, ids), edge_time=conv(t, times), node_x_nids=conv(nids, ids), node_x_time=conv(nt, times),
                node_y_nids=conv(y, ids))  # fmt: skip


def as_batch(step):
    return types.SimpleNamespace(**{k: None if step.get(k) is None else torch.from_numpy(np.array(step[k])) for k in FIELDS})


def pack(arrays, dtypes, name, per_call):
    """per_call: one array or None per call -> `name` (all of them end to end, widened to int64), `name`_len (-1: None); the dtypes go to meta."""
    arrays[name] = np.concatenate([np.asarray(v).astype(I64) for v in per_call if v is not None] + [np.empty(0, dtype=I64)])
    arrays[name + '_len'] = np.array([-1 if v is None else len(v) for v in per_call], dtype=I64)
    dtypes[name] = [None if v is None else str(np.asarray(v).dtype) for v in per_call]


def save(name, meta, arrays, steps, outputs=()):
    calls = [s for s in steps if not isinstance(s, str)]
    dtypes = meta.setdefault('dtypes', {})
    for k in FIELDS:
        pack(arrays, dtypes, k, [s.get(k) for s in calls])
    for k, per_call in outputs:
        pack(arrays, dtypes, k, per_call)
    n = iter(range(len(calls)))
    meta['steps'] = [s if isinstance(s, str) else next(n) for s in steps]
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    size = os.path.getsize(path)
    assert size < 200_000, (name, size)
    print(f'{name}: {size} bytes, {len(calls)} calls')


# ---- g27 -----------------------------------------------------------------------------------------------------------------------------------


def batch_analytics(name, steps):
    hook, out = BatchAnalyticsHook(), []
    for s in steps:
        b = hook(DG, as_batch(s))
        vals = [getattr(b, k) for k in BA_KEYS]
        assert all(type(v) is (float if k == 'avg_degree' else int) for k, v in zip(BA_KEYS, vals)), (name, vals)
        out.append(vals)
    save(f'g27_batch_analytics_{name}', dict(out=out), {}, steps)
    return out


def g27():
    rng = np.random.default_rng(2700)
    out = batch_analytics('unit', [B([1, 1, 2], [2, 2, 3], [1, 1, 2], [2, 2, 3], [5, 5, 6], times=I32)])
    assert out[0] == [3, 3, 4, 3, 2.0, 1, 1]
    batch_analytics('identical', [B(np.full(n, 4), np.full(n, 9), np.full(n, 77), np.full(n, 4), np.full(n, 77)) for n in (1, 63, 64, 65, 200)])
    batch_analytics('distinct', [B(np.arange(n), np.arange(n) + n, np.arange(n), np.arange(n) + 2 * n, np.arange(n) + n) for n in (1, 63, 64, 65, 200)])
    rnd = lambda n, hi=40, thi=30: B(rng.integers(0, hi, n), rng.integers(0, hi, n), np.sort(rng.integers(0, thi, n)), rng.integers(0, hi, n // 2 + 1),
                                     np.sort(rng.integers(0, thi, n // 2 + 1)))  # fmt: skip
    batch_analytics('sizes', [rnd(n) for n in (1, 63, 64, 65, 200)])
    # E = 7 over U = 6 ids: the float32 quotient
    out = batch_analytics('avg_degree_f32', [B([0, 1, 2, 3, 4, 5, 0], [1, 2, 3, 4, 5, 0, 1], np.arange(7))])
    assert out[0][4] == 2.3333332538604736 != 14 / 6, out
    big = 2**24
    t_big = [big, big + 1, 5, big + 2, big + 3, 2 * big + 2, 2 * big + 4]
    ends = ([0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 0])
    out = batch_analytics('time_f32_rounding', [B([0, 1, 2], [1, 2, 0], [big, big + 1, 5]), B(*ends, t_big), B(None, None, None, [0, 1, 2], [big, big + 1, 5]),
                                                B(None, None, None, [3, 3, 3, 3, 3, 3, 3], t_big)])  # fmt: skip
    assert out[0][2] == 2 and out[2][2] == 2, out  # one side None: the times are rounded to float32 before they are counted
    assert out[1][2] < 7 and out[1][5] == 0, out  # ... while the triples compare the times at full width
    out = batch_analytics('time_exact', [B([0, 1, 2], [1, 2, 0], [big, big + 1, 5], [1], [big + 1]), B(*ends, t_big, [], []),
                                         B(*ends, t_big, [9, 9], [2 * big + 3, 2 * big + 5])])  # fmt: skip
    assert out[0][2] == 3 and out[1][2] == 7 and out[2][2] == 9, out  # both present (even empty): exact
    batch_analytics('int32_times', [rnd(50), B([1, 2], [3, 4], [7, 7], times=I32), B([1, 2], [3, 4], [7, 8], [5], [7], times=I32)])
    neg = rnd(60)
    neg['edge_time'], neg['node_x_time'] = neg['edge_time'] - 20, neg['node_x_time'] - 20
    batch_analytics('negative_times', [neg, B([1, 1], [2, 2], [-5, -5]), B([1, 1], [2, 2], [-5, -5], [1], [-6])])
    top = 2**31 - 2
    batch_analytics('large_ids', [B([top, 0, top - 1, top], [0, top, top, 0], [1, 2, 3, 1], [top, top - 1, 7], [1, 1, 1]),
                                  B([top, 5], [top, 5], [2**40, 2**40 + 1], [top], [2**40], ids=I64)])  # fmt: skip
    out = batch_analytics('empty_and_none', [B([], [], [], [], []), B(), B([1, 2, 1], [2, 3, 2], [4, 4, 4]), B(None, None, None, [3, 3, 4], [1, 1, 2]),
                                             B([1, 2, 1], [2, 3, 2], [4, 4, 4], [2, 2], None), B([], [], [], [2, 2], [3, 3]),
                                             B([1, 1], [2, 2], None, [2], [3])])  # fmt: skip
    assert out[0] == [0, 0, 0, 0, 0.0, 0, 0] == out[1], out
    assert out[4][6] == 0 and out[4][1] == 2 and out[6][5] == 0, out  # no node_x_time / no edge_time: no repeats counted


# ---- g28 -----------------------------------------------------------------------------------------------------------------------------------


def seen_nodes(name, num_nodes, steps):
    hook = EdgeEventsSeenNodesTrackHook(num_nodes)
    marked, seen, pos = [], [], []
    for s in steps:
        if isinstance(s, str):
            hook.reset_state()
            assert not hook._seen_mask.any()
            continue
        b = hook(DG, as_batch(s))
        y = s['node_y_nids']
        assert b.batch_nodes_mask.dtype == torch.int64 and b.seen_nodes.dtype == (torch.int32 if y is None else torch.from_numpy(y).dtype), name
        seen.append(b.seen_nodes.numpy().copy())
        pos.append(b.batch_nodes_mask.numpy().copy())
        marked.append(int(hook._seen_mask.sum()))
    save(f'g28_seen_nodes_{name}', dict(num_nodes=num_nodes, marked=marked), dict(mask=hook._seen_mask.numpy().copy()), steps,
         [('seen_nodes', seen), ('batch_nodes_mask', pos)])  # fmt: skip
    return seen, pos


def g28():
    rng = np.random.default_rng(2800)
    # the reference's unit stream, batch_unit='s': times 1..5; edges (2, 3) at 1 and (2, 5) at 5; labels 4 at 2, 2 at 3, {5, 1, 2} at 5
    E = lambda: np.empty(0, dtype=I32)
    seen, pos = seen_nodes('unit', 6, [B([2], [3]), B(E(), E(), y=[4]), B(E(), E(), y=[2]), B(E(), E()), B([2], [5], y=[5, 1, 2])])
    assert seen[2].tolist() == [2] and seen[4].tolist() == [5, 2] and pos[4].tolist() == [0, 2]
    seen, pos = seen_nodes('same_batch_and_repeats', 10, [B([1], [2], y=[3, 1, 1, 2, 3, 1]), B([3], [3], y=[3, 3, 9, 1]), B(E(), E(), y=[9, 9])])
    assert seen[0].tolist() == [1, 1, 2, 1] and pos[0].tolist() == [1, 2, 3, 5]  # first seen in this very batch, repeats kept
    seen, pos = seen_nodes('no_labels', 8, [B([1, 2], [3, 4]), B([5], [6], y=[]), B(E(), E(), y=[1, 5, 7, 6])])
    assert seen[0].dtype == I32 and seen[0].size == 0 and seen[2].tolist() == [1, 5, 6]  # the marking still happened
    steps = []
    for ny in (0, 1, 63, 64, 65, 1025):
        steps.append(B(rng.integers(0, 400, 30), rng.integers(0, 400, 30), y=rng.integers(0, 400, ny)))
    seen_nodes('sizes', 400, steps)
    mk = lambda: B(rng.integers(0, 50, 6), rng.integers(0, 50, 6), y=rng.integers(0, 50, 40))
    seen_nodes('reset', 50, [mk(), mk(), 'reset', mk(), mk()])
    seen_nodes('int64_labels', 50, [B(rng.integers(0, 50, 10), rng.integers(0, 50, 10), y=np.asarray(rng.integers(0, 50, 70), dtype=I64)) for _ in range(3)]
               + [B(np.asarray([49, 0], dtype=I64), np.asarray([0, 49], dtype=I64), y=np.asarray([49, 0, 49], dtype=I64))])  # fmt: skip


# ---- g29 -----------------------------------------------------------------------------------------------------------------------------------


def node_analytics(name, tracked, num_nodes, steps, hook_id=None):
    hook = NodeAnalyticsHook(torch.tensor(tracked), num_nodes, id=hook_id)
    sfx = f'_{hook_id}' if hook_id else ''
    sizes, suffixed, keys, outs = [], [], {}, []
    ids, stats, macros, edges = [], [], [], []
    for s in steps:
        if isinstance(s, str):
            hook.reset_state()
            continue
        b = hook(DG, as_batch(s))
        sfx_now = sfx if hasattr(b, 'node_stats' + sfx) else ''
        suffixed.append(sfx_now == sfx)
        ns, macro, edge = (getattr(b, k + sfx_now) for k in ('node_stats', 'node_macro_stats', 'edge_stats'))
        for what, d in (('macro_keys', macro), ('edge_keys', edge), *(('node_keys', v) for v in ns.values())):
            assert keys.setdefault(what, list(d)) == list(d), (name, what)
        ids.append(np.array(list(ns), dtype=I64))
        stats.append(np.array([[float(v) for v in st.values()] for st in ns.values()], dtype=np.float64).reshape(len(ns), 6))
        assert all(float(v) == v for st in ns.values() for v in st.values())
        macros.append([float(v) for v in macro.values()])
        edges.append([float(v) for v in edge.values()])
        sizes.append([len(hook._total_timesteps), len(hook._seen_edges), sum(map(len, hook._all_neighbors.values())), sum(map(len, hook._node_timesteps.values()))])
        outs.append((ns, macro, edge))
    keys.setdefault('node_keys', ['degree', 'activity', 'new_neighbors', 'lifetime', 'time_since_last_seen', 'appearances'])
    assert keys['node_keys'] == ['degree', 'activity', 'new_neighbors', 'lifetime', 'time_since_last_seen', 'appearances']
    assert keys['macro_keys'] == ['node_novelty', 'new_node_count'] and keys['edge_keys'] == ['edge_novelty', 'edge_density', 'new_edge_count']
    meta = dict(tracked=[int(t) for t in tracked], num_nodes=num_nodes, id=hook_id, sizes=sizes, suffixed=suffixed, **keys)
    arrays = dict(stats=np.concatenate(stats), macro=np.array(macros, dtype=np.float64), edge=np.array(edges, dtype=np.float64))
    save(f'g29_node_analytics_{name}', meta, arrays, steps, [('ids', ids)])
    return outs


def g29():
    rng = np.random.default_rng(2900)
    # the reference's 9-edge graph, in the slices its tests take
    src, dst, t = [0, 0, 1, 2, 1, 3, 2, 0, 4], [1, 2, 2, 3, 0, 4, 1, 3, 0], [0, 0, 1, 1, 2, 2, 3, 3, 4]
    sl = lambda a, b: B(src[a:b], dst[a:b], t[a:b], times=I32)
    outs = node_analytics('unit', [0, 1, 2], 5, [sl(0, 2), sl(2, 4), sl(4, 6), sl(6, 8), sl(8, 9), sl(0, 2)])
    assert outs[0][0][0] == dict(degree=2, activity=1.0, new_neighbors=2, lifetime=0, time_since_last_seen=0.0, appearances=1)
    assert list(outs[1][0]) == [1, 2, 0] and outs[5][2]['new_edge_count'] == 0  # present ascending, then the absent ones
    node_analytics('unit_with_id', [0, 3, 3], 5, [sl(0, 2), sl(2, 4), sl(4, 9)], hook_id='foo')
    # 40 batches of 50 edges over 300 nodes
    st = make_stream('wiki', seed=2901, num_edges=2000, n_src=180, n_dst=120, edge_dim=0)
    s_, d_, t_ = st.src.numpy().astype(I64), st.dst.numpy().astype(I64), st.ts.numpy().astype(I64)
    assert int(max(s_.max(), d_.max())) < 300 and t_.min() >= 0
    stream = [B(s_[a : a + 50], d_[a : a + 50], t_[a : a + 50], rng.integers(0, 300, 5), np.full(5, t_[a + 49])) for a in range(0, 2000, 50)]
    for T in (1, 3, 64, 65, 300):  # (all 300 tracked: a row per node seen and call, so the first 10 calls only, to keep the file small)
        node_analytics(f'stream_T{T}', sorted(rng.choice(300, T, replace=False).tolist()), 300, stream[: 10 if T == 300 else 40])
    hub = [B(np.full(20, 7), rng.integers(0, 30, 20), np.arange(c * 20, c * 20 + 20)) for c in range(3)] + [B(rng.integers(0, 30, 20), np.full(20, 7), np.full(20, 70))]
    node_analytics('hub', [7, 3], 30, hub)
    outs = node_analytics('self_loops', [1, 2], 4, [B([1, 1, 2], [1, 1, 3], [5, 6, 6]), B([2, 1], [2, 0], [7, 7])])
    assert outs[0][0][1]['degree'] == 4 and outs[0][0][1]['new_neighbors'] == 1 and outs[1][0][2]['new_neighbors'] == 1  # a self loop: degree 2, its own neighbour
    outs = node_analytics('repeated_pairs', [0], 6, [B([0, 0, 1, 0], [1, 1, 0, 1], [1, 1, 2, 3]), B([0, 2, 0], [1, 3, 1], [4, 4, 5]), B([1], [0], [6])])
    assert [o[2]['new_edge_count'] for o in outs] == [2, 1, 0] and outs[0][2]['edge_novelty'] == 0.5  # repeated inside the batch: counted once
    # node events only, edges only, an empty batch in between, the all-None batch, node events of untracked ids
    E = lambda dt=I32: np.empty(0, dtype=dt)
    mixed = [B(None, None, None, [0, 1, 2, 5, 5], [3, 3, 4, 4, 4]), B([0, 4], [1, 5], [6, 7]), B(E(), E(), E(I64)), B([1], [2], [9], [5, 4, 0], [9, 9, 9]),
             B(), B(E(), E(), E(I64), [4, 5, 5], [12, 12, 13]), B([2, 2], [0, 0], [14, 15], [2], None)]  # fmt: skip
    outs = node_analytics('mixed_batches', [0, 1, 2], 6, mixed)
    assert outs[0][1] == dict(node_novelty=0.4, new_node_count=2)  # the untracked ids 5, 5 -- though every id of the batch is new
    assert outs[3][1] == dict(node_novelty=2 / 3, new_node_count=2) and outs[5][1] == dict(node_novelty=1.0, new_node_count=3)
    assert [outs[2][0][n]['time_since_last_seen'] for n in (0, 1, 2)] == [-7, -7, -4]  # an empty batch: current_time is 0
    assert outs[4] == ({}, dict(node_novelty=0.0, new_node_count=0), dict(edge_novelty=0.0, edge_density=0.0, new_edge_count=0))
    node_analytics('all_none_with_id', [0], 3, [B([0], [1], [1]), B(), B([0], [2], [2])], hook_id='bar')
    node_analytics('reset', [1, 2, 3], 8, [sl(0, 4), sl(4, 9), 'reset', sl(0, 4), sl(2, 6)])


def check_unsuffixed():
    hook = NodeAnalyticsHook(torch.tensor([0]), 3, id='bar')
    b = hook(DG, as_batch(B()))
    assert hasattr(b, 'node_stats') and not hasattr(b, 'node_stats_bar')  # all None: written without the id suffix
    try:
        NodeAnalyticsHook(torch.tensor([0]), 3)(DG, as_batch(B([0], [3], [1])))
    except IndexError:
        pass
    else:
        raise AssertionError('an id >= num_nodes should raise IndexError')


if __name__ == '__main__':
    torch.set_num_threads(1)
    check_unsuffixed()
    g27()
    g28()
    g29()
