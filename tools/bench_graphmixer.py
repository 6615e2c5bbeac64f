#!/usr/bin/env python
"""GraphMixer at the cfg-2 shape (wiki-shaped stream, bs 200, k = [20], time_gap 2000, node_dim 100, embed 128, two mixer layers):
TimeGapNeighborHook per batch, the native encoder forward per batch against the same forward composed from torch ops on the same
device, and the example-style Python hook on the host (a reference point only).  Each figure is the median of three windows.
Prints one JSON line.   python tools/bench_graphmixer.py [--edges E] [--batches B]"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook, TimeGapNeighborHook  # noqa: E402
from tgm_amd.nn import GraphMixerEncoder  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

PEAK_TF = 157.3  # MI355X fp32 MFMA, dense

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=60_000)
ap.add_argument('--batches', type=int, default=40, help='batches per timed window')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, gap, F_, E_, T = 200, 20, 2000, 100, 128, 100
s = make_stream('wiki', num_edges=args.edges)
N, D = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
node_feat = torch.randn(N, F_, device=dev)
tg_hook = TimeGapNeighborHook(gap)
hm = HookManager(keys=['k'])
hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
hm.register('k', tg_hook)
loader = DGDataLoader(dg, batch_size=bs, hook_manager=hm)
with hm.activate('k'):
    batches = [b for _, b in zip(range(len(loader)), loader)]
starts = list(loader._starts)
# steady-state batches: full windows behind them (skip the warm-up of the recency buffers and of the time gap)
skip = max(gap // bs + 1, len(batches) - args.batches - 1)
work = [(dg.slice_events(st, st + bs), b) for st, b in zip(starts, batches)][skip : skip + args.batches]
work = [(v, b) for v, b in work if b.edge_src.numel() == bs]
torch.manual_seed(0)
enc = GraphMixerEncoder(time_dim=T, embed_dim=E_, num_tokens=K, node_dim=F_, edge_dim=D, dropout=0.1).to(dev).eval()


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for v, b in work:
        fn(v, b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(work) * 1e6


def median3(fn):
    window(fn)  # warm-up
    return statistics.median(window(fn) for _ in range(3))


with torch.no_grad():
    hook_us = median3(lambda v, b: tg_hook(v, b))

    def native(v, b):
        enc(b, node_feat)

    def composed(v, b):
        enc._torch_forward(enc._inputs(b, node_feat))

    fwd_us = median3(native)
    torch_us = median3(composed)

# the example's hook on the host: a dict of lists over the window's edges, one list per seed
st = dg._storage
src_h, dst_h = s.src.numpy(), s.dst.numpy()


def host_hook(v, b):
    lo, hi = tg_hook.window(v)
    table = defaultdict(list)
    for u, w in zip(src_h[lo:hi].tolist(), dst_h[lo:hi].tolist()):
        table[u].append(w)
        table[w].append(u)
    seeds = torch.cat([b.edge_src, b.edge_dst, b.neg]).tolist()
    return [table.get(n, []) for n in seeds]


host_us = median3(host_hook)
S, R = 3 * bs, 3 * bs * K
Hc, Ht = int(4.0 * D), int(0.5 * K)
flop = 2 * R * (D + T) * D + 2 * (2 * R * D * Hc * 2 + 2 * S * D * K * Ht * 2) + 2 * S * (D + F_) * E_
gflop = flop / 1e9
print(json.dumps({
    'bench': 'graphmixer_cfg2', 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs, 'k': K,
    'time_gap': gap, 'edge_dim': D, 'time_dim': T, 'node_dim': F_, 'embed_dim': E_, 'window_edges_median': statistics.median(
        tg_hook.window(v)[1] - tg_hook.window(v)[0] for v, _ in work),
    'hook_us_per_batch': round(hook_us, 1), 'forward_us_per_batch': round(fwd_us, 1), 'gflop_per_batch': round(gflop, 3),
    'fraction_of_fp32_mfma_peak': round(gflop * 1e3 / fwd_us / PEAK_TF, 3), 'floor_us_at_peak': round(gflop * 1e3 / PEAK_TF, 1),
    'torch_composed_forward_us_per_batch': round(torch_us, 1), 'native_speedup_vs_torch': round(torch_us / fwd_us, 2),
    'example_style_host_hook_us_per_batch': round(host_us, 1),
}))  # fmt: skip
