#!/usr/bin/env python
"""BatchAnalyticsHook, EdgeEventsSeenNodesTrackHook and NodeAnalyticsHook per batch, in microseconds, on two shapes:

  wiki      the wiki-shaped stream, bs = 200
  comment   the comment-shaped stream (1 000 000 nodes), bs = 4096, its first --comment-edges events

Every batch carries, besides its edges, bs / 4 node events (ids of the batch's destinations, at the batch's last time) and bs / 4 labels.
Measured in the same process:

  native     the hooks of tgm_amd.hooks on device tensors (csrc/analytics.hip): BatchAnalyticsHook with sync=True (one read) and sync=False
             (none), the tracker (one read), NodeAnalyticsHook with --tracked tracked nodes (one read)
  composed   the hooks' definitions from stock torch ops on the device, written here, with the reference's number of device round trips:
             for the batch statistics five sort-based ``unique`` calls whose sizes the host waits for; for the tracker a ``unique``, a
             fill of the mask, a lookup and a ``nonzero``.  (NodeAnalyticsHook has no such form: the reference loops over the events in
             Python; its host-path restatement here is timed on host copies of the same batches instead.)

A timed window is K consecutive batches between two device synchronisations, on a host clock; each figure is the median of --windows
windows with the spread beside it.  The steps (one hook, one way, one shape) run one after another, each with a new hook and five batches to
warm it; a step stops taking windows once --step-seconds have gone by and says how many it took.  Appends one JSON line per shape to --out.
    python tools/bench_analytics.py [--out FILE] [--shapes wiki,comment]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgm_amd.hooks import BatchAnalyticsHook, EdgeEventsSeenNodesTrackHook, NodeAnalyticsHook  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_bench_analytics.jsonl'))
ap.add_argument('--shapes', default='wiki,comment')
ap.add_argument('--comment-edges', type=int, default=1_000_000)
ap.add_argument('--windows', type=int, default=9)
ap.add_argument('--tracked', type=int, default=64)
ap.add_argument('--step-seconds', type=float, default=60.0)
ap.add_argument('--rehearse-on-cpu', action='store_true', help='run the script on host tensors at whatever size is given: checks the script, times nothing of interest, writes no file')
args = ap.parse_args()

if args.rehearse_on_cpu:
    dev = torch.device('cpu')
    sync = lambda: None
else:
    assert torch.cuda.is_available(), 'bench_analytics.py measures on a ROCm device'
    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize
DG = types.SimpleNamespace(device=dev)


def composed_batch_analytics(b):
    """the seven statistics as the hook's docstring defines them, each distinct count its own sort-based ``unique`` whose size the host
    waits for (five of them, as many device round trips as the reference makes for these fields)"""
    distinct = lambda *cols: torch.cat(cols).unique().shape[0]
    distinct_rows = lambda *cols: torch.stack(cols, 1).unique(dim=0).shape[0]
    E, Nn = b.edge_src.shape[0], b.node_x_nids.shape[0]
    u_edge = distinct(b.edge_src, b.edge_dst)
    avg = (torch.tensor(2 * E, dtype=torch.float32) / torch.tensor(u_edge, dtype=torch.float32)).item() if E else 0.0
    return (E, Nn, distinct(b.edge_time, b.node_x_time), distinct(b.edge_src, b.edge_dst, b.node_x_nids), avg,
            E - distinct_rows(b.edge_src, b.edge_dst, b.edge_time), Nn - distinct_rows(b.node_x_nids, b.node_x_time))  # fmt: skip


class ComposedTracker:
    """the tracker's definition from torch ops: distinct endpoints marked, the labels looked up, the marked positions compacted"""

    def __init__(self, num_nodes):
        self.mask = torch.zeros(num_nodes, dtype=torch.bool, device=dev)

    def __call__(self, b):
        self.mask.index_fill_(0, torch.cat([b.edge_src, b.edge_dst]).unique().long(), True)
        pos = self.mask.index_select(0, b.node_y_nids.long()).nonzero().view(-1)
        return pos, b.node_y_nids.index_select(0, pos)


def spread(v):
    return {'median': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1), 'windows': len(v)}


def run(shape: str, bs: int, edges: int, K: int) -> dict:
    s = make_stream(shape, num_edges=edges, edge_dim=0)
    N = s.num_nodes
    src, dst, ts = s.src.to(dev), s.dst.to(dev), s.ts.to(dev)
    per_pass, q = edges // bs, max(1, bs // 4)
    labels = torch.randint(0, N, (edges,), dtype=torch.int32, generator=torch.Generator().manual_seed(18)).to(dev)

    def batch(i, to=None):
        lo = (i % per_pass) * bs
        b = types.SimpleNamespace(edge_src=src[lo : lo + bs], edge_dst=dst[lo : lo + bs], edge_time=ts[lo : lo + bs], node_x_nids=dst[lo : lo + q],
                                  node_x_time=ts[lo + bs - 1 : lo + bs].expand(q).contiguous(), node_y_nids=labels[lo : lo + q])  # fmt: skip
        return b if to is None else types.SimpleNamespace(**{k: v.to(to) for k, v in vars(b).items()})

    def windows(step, make_batch=batch, warm=5):
        for i in range(warm):
            step(make_batch(i))
        out, nxt, t_end = [], warm, time.perf_counter() + args.step_seconds
        while len(out) < args.windows and (not out or time.perf_counter() < t_end):
            batches = [make_batch(i) for i in range(nxt, nxt + K)]
            sync()
            t0 = time.perf_counter()
            for b in batches:
                step(b)
            sync()
            out.append((time.perf_counter() - t0) / K * 1e6)
            nxt += K
        return out

    tracked = torch.unique(dst[: 50 * bs])[: args.tracked].cpu()
    steps = {
        'batch_analytics_native_sync': lambda: (lambda h: lambda b: h(DG, b))(BatchAnalyticsHook()),
        'batch_analytics_native_nosync': lambda: (lambda h: lambda b: h(DG, b))(BatchAnalyticsHook(sync=False)),
        'batch_analytics_composed': lambda: composed_batch_analytics,
        'seen_nodes_native': lambda: (lambda h: lambda b: h(DG, b))(EdgeEventsSeenNodesTrackHook(N)),
        'seen_nodes_composed': lambda: ComposedTracker(N),
        'node_analytics_native': lambda: (lambda h: lambda b: h(DG, b))(NodeAnalyticsHook(tracked, N)),
    }
    result = {k: spread(windows(make())) for k, make in steps.items()}
    if shape == 'wiki':  # the host-path restatement on host copies of the batches (the copies are made outside the window)
        host = NodeAnalyticsHook(tracked, N)
        result['node_analytics_host_path'] = spread(windows(lambda b: host(types.SimpleNamespace(device=torch.device('cpu')), b), lambda i: batch(i, 'cpu')))
    # the two ways agree on a batch, before anything is reported
    b = batch(3)
    native = BatchAnalyticsHook()(DG, types.SimpleNamespace(**vars(b)))
    keys = ('num_edge_events', 'num_node_events', 'num_unique_timestamps', 'num_unique_nodes', 'avg_degree', 'num_repeated_edge_events', 'num_repeated_node_events')
    agree = tuple(getattr(native, k) for k in keys) == composed_batch_analytics(b)
    med = {k: v['median'] for k, v in result.items()}
    return {
        'bench': 'analytics_hooks', 'shape': shape, 'device': torch.cuda.get_device_name(0) if dev.type == 'cuda' else 'cpu (rehearsal)', 'bs': bs,
        'node_events_per_batch': q, 'labels_per_batch': q, 'tracked_nodes': int(tracked.numel()), 'num_nodes': N, 'batches_per_window': K,
        'batch_statistics_agree': bool(agree),
        'batch_analytics_speedup_sync': round(med['batch_analytics_composed'] / med['batch_analytics_native_sync'], 1),
        'batch_analytics_speedup_nosync': round(med['batch_analytics_composed'] / med['batch_analytics_native_nosync'], 1),
        'seen_nodes_speedup': round(med['seen_nodes_composed'] / med['seen_nodes_native'], 1),
        'us_per_batch': result,
    }  # fmt: skip


SHAPES = {'wiki': (200, 157_474, 50), 'comment': (4096, args.comment_edges, 20)}
for name in args.shapes.split(','):
    bs, edges, K = SHAPES[name]
    line = json.dumps(run(name, bs, edges, K))
    print(line, flush=True)
    if not args.rehearse_on_cpu:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')
