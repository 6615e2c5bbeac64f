#!/usr/bin/env python
"""DyGFormer at the example's shape (wiki-shaped stream, bs 200, k = [31] so L = 32, patch 1, channel 50, two heads, two layers, node 128,
time 100, out 172): the sampler per batch, and the encoder forward per batch -- the positive and the negative call together, as the
example's evaluation step makes them -- through ``encode_pairs`` (hop 0 read in place), through ``forward`` on gathered tensors (the
gathers timed with it), and composed from torch ops on the same device in the same process.  A timed window loops over the batch list
until it lasts at least --window-s seconds; the three forwards take turns (one window each, three rounds, after a warm-up window each)
and each figure is the median of its three windows.  Prints one JSON line.   python tools/bench_dygformer.py [--edges E] [--batches B]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import DyGFormer  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

PEAK_TF = 157.3  # MI355X fp32 MFMA, dense

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=60_000)
ap.add_argument('--batches', type=int, default=40, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, dN, dT, C, E_, H, NL = 200, 31, 128, 100, 50, 172, 2, 2
s = make_stream('wiki', num_edges=args.edges)
N, dE = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
node_x = torch.randn(N, dN, device=dev)


def make_loader():
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
    hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    return hm, DGDataLoader(dg, batch_size=bs, hook_manager=hm)


def sampler_window():
    hm, loader = make_loader()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with hm.activate('k'):
        n = sum(1 for _ in loader)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


sampler_window()  # warm-up
sampler_us = statistics.median(sampler_window() for _ in range(3))

hm, loader = make_loader()
with hm.activate('k'):
    batches = list(loader)
work = [b for b in batches if b.edge_src.numel() == bs][-args.batches :]  # steady state: full neighbour windows
torch.manual_seed(0)
enc = DyGFormer(node_feat_dim=dN, edge_x_dim=dE, time_feat_dim=dT, channel_embedding_dim=C, output_dim=E_, patch_size=1, num_layers=NL, num_heads=H,
                dropout=0.1, max_input_sequence_length=K + 1, device=dev).to(dev).eval()  # fmt: skip
ar = torch.arange(bs, device=dev, dtype=torch.int32)
ROWS = {False: (ar, ar + bs), True: (ar, ar + 2 * bs)}


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for b in work:
            fn(b, False)
            fn(b, True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * len(work)) * 1e6


def alternating_medians(fns):
    """Warm each up (which also sizes its window), then one window each in turn, three rounds: drift of the device hits all alike."""
    for fn in fns:
        window(fn)  # warm-up (first-call costs would undersize the window below)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / (window(fn) * len(work)))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [round(r * len(work) * statistics.median(v) / 1e6, 2) for r, v in zip(reps, seen)]


def pairs(b, neg):
    sr, dr = ROWS[neg]
    return enc.encode_pairs(node_x, b.edge_src, b.neg if neg else b.edge_dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr)


def gathered(b, neg):
    rows = torch.cat(ROWS[neg]).long()
    return enc(node_x, torch.stack([b.edge_src, b.neg if neg else b.edge_dst]), b.edge_time, b.nbr_nids[0][rows], b.nbr_edge_time[0][rows],
               b.nbr_edge_x[0][rows])  # fmt: skip


def composed(b, neg):
    sr, dr = ROWS[neg]
    return enc._torch_forward(enc._inputs(node_x, b.edge_src, b.neg if neg else b.edge_dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0],
                                          b.nbr_edge_x[0], sr, dr))  # fmt: skip


with torch.no_grad():
    (pairs_us, gathered_us, torch_us), window_s = alternating_medians([pairs, gathered, composed])

L, P = K + 1, bs
R, D = 2 * P * L, 4 * C  # token rows of one call (patch 1), model width
flop_call = 2 * R * (dN + dE + dT + C) * C + NL * (2 * R * D * 3 * D + 2 * R * D * D + 2 * 2 * R * D * 4 * D + 2 * 2 * P * H * (2 * L) ** 2 * (D // H)) + 2 * 2 * P * D * E_
gflop = 2 * flop_call / 1e9  # the positive and the negative call
print(json.dumps({
    'bench': 'dygformer_example_shape', 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs, 'k': K,
    'edge_dim': dE, 'node_dim': dN, 'time_dim': dT, 'channel_dim': C, 'heads': H, 'layers': NL, 'out_dim': E_,
    'sampler_us_per_batch': round(sampler_us, 1), 'forward_encode_pairs_us_per_batch': round(pairs_us, 1),
    'forward_gathered_us_per_batch': round(gathered_us, 1), 'torch_composed_forward_us_per_batch': round(torch_us, 1),
    'native_speedup_vs_torch': round(torch_us / pairs_us, 2), 'gflop_per_batch': round(gflop, 2),
    'fraction_of_fp32_mfma_peak': round(gflop * 1e3 / pairs_us / PEAK_TF, 3), 'floor_us_at_peak': round(gflop * 1e3 / PEAK_TF, 1),
    'window_seconds': window_s,
}))  # fmt: skip
