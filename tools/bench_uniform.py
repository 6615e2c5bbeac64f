#!/usr/bin/env python
"""NeighborSamplerHook (uniform temporal neighbor sampling, tgm/hooks/neighbors/uniform.py:87-142) at the headline shape: wiki-shaped stream,
seeds = src | dst | neg, num_nbrs = [20, 20], bs = 200; steady-state batches mid-stream, HIP events around the timed steps; one JSON line.
python tools/bench_uniform.py [n_steps]

python tools/bench_uniform.py [n_steps] --k 128 512 [--out FILE]: one hop of k neighbours instead (past 64: tgmx_uniform_lookup_wide), next to
RecencyNeighborHook(mode='csr') at the same k, which writes the same output bytes.  Both with validate='deferred' (no device -> host read per
batch); the two take turns in one process -- a warm-up window each, then one window of n_steps batches each, three rounds -- and each figure
is the median of its three windows, a host clock around work that ends in a device synchronise.  One JSON line per k; --out appends them."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import HookManager, NeighborSamplerHook, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('n_steps', nargs='?', type=int, default=200)
ap.add_argument('--k', nargs='+', type=int, default=None, help='one hop of k neighbours, next to the recency sampler (mode=csr) at the same k')
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
n = args.n_steps
KEYS = (['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time'])


def one_hop(k: int) -> dict:
    bs = 200
    st = make_stream('wiki', seed=1337)
    dg = DGraph(DGData.from_raw(st.ts, torch.stack([st.src, st.dst], 1), st.edge_x, static_node_x=st.node_x), device=dev)
    runs = {}
    for name, sampler in (('uniform', NeighborSamplerHook([k], *KEYS, seed=7, validate='deferred')),
                          ('recency_csr', RecencyNeighborHook(st.num_nodes, [k], *KEYS, mode='csr', validate='deferred', batch_size=bs))):  # fmt: skip
        hm = HookManager(keys=['k'])
        hm.register('k', RandomNegativeEdgeSamplerHook(int(st.dst.min()), st.num_nodes))
        hm.register('k', sampler)
        loader = DGDataLoader(dg, batch_size=bs, hook_manager=hm)
        runs[name] = (hm, loader, sampler)
    first = len(runs['uniform'][1]._starts) // 2
    span = len(runs['uniform'][1]._starts) - first

    def window(name: str) -> float:
        hm, loader, sampler = runs[name]
        with hm.activate('k'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(n):
                loader(loader._starts[first + t % span])  # (the second half of the stream, again from its start when n_steps is larger)
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / n * 1e6
            sampler.check()
        return us

    seen = {name: [] for name in runs}
    for name, (hm, loader, _) in runs.items():
        with hm.activate('k'):
            loader(loader._starts[0])  # the recency hook anchors its epoch at the first batch it sees: the stream's first, so mid-stream it sees the history
        window(name)
    for _ in range(3):
        for name in runs:
            seen[name].append(window(name))
    med = {name: statistics.median(v) for name, v in seen.items()}
    return {'what': 'one hop of k neighbours, wiki-shaped stream, bs 200, seeds src | dst | neg, dense feature rows, validate=deferred; us per batch, '
                    'median of three alternating windows of n_steps mid-stream batches', 'k': k, 'n_steps': n, 'D': int(st.edge_dim),
            'out_bytes_per_batch': 3 * bs * k * (4 + 8 + 4 * int(st.edge_dim)), 'uniform_us': round(med['uniform'], 1),
            'recency_csr_us': round(med['recency_csr'], 1), 'windows': {name: [round(x, 1) for x in v] for name, v in seen.items()}}  # fmt: skip


if args.k:
    for k in args.k:
        line = json.dumps(one_hop(k))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    sys.exit(0)

res = {}
for shape, bs, ks, validate in (('wiki', 200, [20, 20], 'sync'), ('wiki', 200, [20, 20], 'deferred'), ('review', 512, [10, 10], 'sync'),
                               ('review', 512, [10, 10], 'deferred')):
    st = make_stream(shape, seed=1337)
    dg = DGraph(DGData.from_raw(st.ts, torch.stack([st.src, st.dst], 1), st.edge_x, static_node_x=st.node_x), device=dev)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(int(st.dst.min()), st.num_nodes))
    hm.register('k', NeighborSamplerHook(ks, ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time'], seed=7, validate=validate))
    loader = DGDataLoader(dg, batch_size=bs, hook_manager=hm)
    starts = loader._starts
    first = len(starts) // 2
    with hm.activate('k'):
        for i in range(first, first + 30):
            b = loader(starts[i])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(first + 30, first + 30 + n):
            b = loader(starts[i])
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        hm.active_hooks()[-1].check()
    us = e0.elapsed_time(e1) / n * 1000
    slots = 3 * bs * ks[0] + 3 * bs * ks[0] * ks[1]
    res[f'{shape}, validate={validate}'] = {'us_per_batch': us, 'host_us_per_batch': 1e6 * (t1 - t0) / n, 'sampled_edges_per_s': slots / (us * 1e-6), 'bs': bs, 'num_nbrs': ks,
                  'slots_per_batch': slots, 'D': int(st.edge_dim)}
print(json.dumps({'what': 'NeighborSamplerHook (uniform sampling over the static index, dense feature rows) behind DGDataLoader, steady-state batches mid-stream', **res}))
