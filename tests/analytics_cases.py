"""Shared by tests/test_analytics_cpu.py and tests/test_analytics_gpu.py: the g27 / g28 / g29 fixtures as step lists, replays of them on
whatever device is asked for (asserting everything the fixture records), and the generated streams both files run."""
from __future__ import annotations

import glob
import os
import types

import numpy as np
import torch

import golden_util
from tgm_amd.hooks import BatchAnalyticsHook, EdgeEventsSeenNodesTrackHook, NodeAnalyticsHook

FIELDS = ('edge_src', 'edge_dst', 'edge_time', 'node_x_nids', 'node_x_time', 'node_y_nids')
BA_KEYS = ('num_edge_events', 'num_node_events', 'num_unique_timestamps', 'num_unique_nodes', 'avg_degree', 'num_repeated_edge_events',
           'num_repeated_node_events')  # fmt: skip
NODE_KEYS = ['degree', 'activity', 'new_neighbors', 'lifetime', 'time_since_last_seen', 'appearances']
EXPECTED = {
    'g27_batch_analytics': ['unit', 'identical', 'distinct', 'sizes', 'avg_degree_f32', 'time_f32_rounding', 'time_exact', 'int32_times', 'negative_times',
                            'large_ids', 'empty_and_none'],
    'g28_seen_nodes': ['unit', 'same_batch_and_repeats', 'no_labels', 'sizes', 'reset', 'int64_labels'],
    'g29_node_analytics': ['unit', 'unit_with_id', 'stream_T1', 'stream_T3', 'stream_T64', 'stream_T65', 'stream_T300', 'hub', 'self_loops', 'repeated_pairs',
                           'mixed_batches', 'all_none_with_id', 'reset'],
}  # fmt: skip


def fixtures(prefix: str):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_util.GOLDEN_DIR, prefix + '_*.npz')))


def dg_on(device) -> types.SimpleNamespace:
    """What the hooks read of a graph: its device."""
    return types.SimpleNamespace(device=torch.device(device))


def unpack(meta, a, name):
    """The per-call vectors of a packed field: [array in its recorded dtype, or None]."""
    out, lo = [], 0
    for n, dt in zip(a[name + '_len'].tolist(), meta['dtypes'][name]):
        out.append(None if n < 0 else a[name][lo : lo + n].astype(dt))
        lo += max(n, 0)
    return out


def load(name: str):
    """-> meta, arrays, steps: 'reset' or (call number, {field: array or None})"""
    meta, a = golden_util.load(name)
    per_field = {k: unpack(meta, a, k) for k in FIELDS}
    steps = [s if isinstance(s, str) else (s, {k: per_field[k][s] for k in FIELDS}) for s in meta['steps']]
    return meta, a, steps


def batch_of(fields: dict, device):
    return types.SimpleNamespace(**{k: None if fields.get(k) is None else torch.from_numpy(np.array(fields[k])).to(device) for k in FIELDS})


def B(src=None, dst=None, t=None, nids=None, nt=None, y=None, ids=np.int32, times=np.int64) -> dict:
    conv = lambda v, dt: None if v is None else np.asarray(v, dtype=dt)
    return dict(edge_src=conv(src, ids), edge_dst=conv(dst, ids), edge_time=conv(t, times), node_x_nids=conv(nids, ids), node_x_time=conv(nt, times),
                node_y_nids=conv(y, ids))  # fmt: skip


# ---- BatchAnalyticsHook ----------------------------------------------------------------------------------------------------------------


def batch_analytics_values(batch, sfx='') -> list:
    return [getattr(batch, k + sfx) for k in BA_KEYS]


def run_batch_analytics(batches, device, **kw) -> list:
    hook, dg = BatchAnalyticsHook(**kw), dg_on(device)
    return [batch_analytics_values(hook(dg, batch_of(b, device))) for b in batches]


def replay_batch_analytics(name: str, device) -> list:
    meta, _, steps = load(name)
    out = run_batch_analytics([f for _, f in steps], device)
    for i, (got, want) in enumerate(zip(out, meta['out'])):
        assert got == want, f'{name} call {i}: {got} != {want}'
        assert all(type(v) is (float if k == 'avg_degree' else int) for k, v in zip(BA_KEYS, got)), f'{name} call {i}: {got}'
    return out


# ---- EdgeEventsSeenNodesTrackHook ------------------------------------------------------------------------------------------------------


def run_seen_nodes(num_nodes: int, steps, device, hook=None):
    """steps: 'reset' or a field dict -> hook, [(seen_nodes, batch_nodes_mask) on the host]"""
    hook, dg, out = hook or EdgeEventsSeenNodesTrackHook(num_nodes), dg_on(device), []
    for s in steps:
        if isinstance(s, str):
            hook.reset_state()
            assert not hook._seen_mask.any()
            continue
        b = hook(dg, batch_of(s, device))
        assert b.seen_nodes.device.type == b.batch_nodes_mask.device.type == torch.device(device).type
        out.append((b.seen_nodes.cpu(), b.batch_nodes_mask.cpu()))
    return hook, out


def replay_seen_nodes(name: str, device):
    meta, a, steps = load(name)
    hook, out = run_seen_nodes(meta['num_nodes'], [s if isinstance(s, str) else s[1] for s in steps], device)
    seen, pos = unpack(meta, a, 'seen_nodes'), unpack(meta, a, 'batch_nodes_mask')
    for i, (got_seen, got_pos) in enumerate(out):
        assert str(got_seen.dtype)[6:] == meta['dtypes']['seen_nodes'][i] and got_pos.dtype == torch.int64, f'{name} call {i}'
        assert got_seen.tolist() == seen[i].tolist() and got_pos.tolist() == pos[i].tolist(), f'{name} call {i}'
    assert hook._seen_mask.dtype == torch.bool and np.array_equal(hook._seen_mask.cpu().numpy(), a['mask']), name
    return hook, out


def assert_same_seen(a, b, what: str) -> None:
    assert len(a) == len(b)
    for i, ((s0, p0), (s1, p1)) in enumerate(zip(a, b)):
        assert s0.dtype == s1.dtype and torch.equal(s0, s1) and p0.dtype == p1.dtype == torch.int64 and torch.equal(p0, p1), f'{what} call {i}'


# ---- NodeAnalyticsHook -----------------------------------------------------------------------------------------------------------------


def run_node_analytics(tracked, num_nodes: int, steps, device, hook_id=None, hook=None, **kw):
    """-> hook, [(node_stats, node_macro_stats, edge_stats, suffixed)]"""
    hook = hook or NodeAnalyticsHook(torch.tensor(tracked), num_nodes, id=hook_id, **kw)
    dg, out, sfx = dg_on(device), [], f'_{hook_id}' if hook_id else ''
    for s in steps:
        if isinstance(s, str):
            hook.reset_state()
            continue
        b = hook(dg, batch_of(s, device))
        now = sfx if hasattr(b, 'node_stats' + sfx) else ''
        out.append((getattr(b, 'node_stats' + now), getattr(b, 'node_macro_stats' + now), getattr(b, 'edge_stats' + now), now == sfx))
    return hook, out


def replay_node_analytics(name: str, device, **kw):
    meta, a, steps = load(name)
    hook, out = run_node_analytics(meta['tracked'], meta['num_nodes'], [s if isinstance(s, str) else s[1] for s in steps], device, hook_id=meta['id'], **kw)
    assert hook.tracked_nodes.tolist() == sorted(set(meta['tracked'])) and hook.num_nodes == meta['num_nodes']
    ids, lo = unpack(meta, a, 'ids'), 0
    for i, (ns, macro, edge, suffixed) in enumerate(out):
        where = f'{name} call {i}'
        assert suffixed == meta['suffixed'][i], where
        assert list(ns) == ids[i].tolist(), f'{where}: node order {list(ns)} != {ids[i].tolist()}'
        for r, (n, st) in enumerate(ns.items()):
            assert list(st) == meta['node_keys'] == NODE_KEYS, where
            assert list(st.values()) == a['stats'][lo + r].tolist(), f'{where} node {n}: {st} != {a["stats"][lo + r].tolist()}'
        lo += len(ns)
        assert list(macro) == meta['macro_keys'] and list(macro.values()) == a['macro'][i].tolist(), f'{where}: {macro}'
        assert list(edge) == meta['edge_keys'] and list(edge.values()) == a['edge'][i].tolist(), f'{where}: {edge}'
    st = hook.state()
    assert [len(st[k]) for k in ('times', 'edges', 'nbrs', 'apps')] == meta['sizes'][-1], name
    return hook, out


def assert_same_node_runs(a, b, what: str) -> None:
    """dict == dict compares numbers by value (2 == 2.0); the order of the keys is compared on its own"""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, f'{what} call {i}: {x} != {y}'
        assert list(x[0]) == list(y[0]) and all(list(x[0][n]) == list(y[0][n]) for n in x[0]), f'{what} call {i}: key order'


# ---- generated streams (device against host) -------------------------------------------------------------------------------------------

EDGE_SIZES = (0, 1, 63, 64, 65, 1024, 1025, 5000)


def sized_batches(seed: int, num_nodes: int, ids=np.int32, labels: bool = False):
    """One batch per size in EDGE_SIZES twice over (E and Nn / Ny run against each other: E = 0 meets Nn = 5000), times non-decreasing over the stream."""
    rng = np.random.default_rng(seed)
    out, t0 = [], 0
    for E, Nn in zip(EDGE_SIZES + EDGE_SIZES[::-1], EDGE_SIZES[::-1] + EDGE_SIZES):
        span = max(1, (E + Nn) // 3)  # repeated times
        draw = lambda n: rng.integers(0, num_nodes, n)
        cols = [draw(E), draw(E), np.sort(rng.integers(t0, t0 + span, E)), draw(Nn), np.sort(rng.integers(t0, t0 + span, Nn))]
        for group, n in ((cols[:3], E), (cols[3:], Nn)):  # a quarter of the events repeat another one of the batch whole
            to, frm = rng.integers(0, max(n, 1), n // 4), rng.integers(0, max(n, 1), n // 4)
            for c in group:
                c[to] = c[frm]
        b = B(*cols, draw(Nn) if labels else None, ids=ids)
        t0 += span
        out.append(b)
    return out
