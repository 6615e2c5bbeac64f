#!/usr/bin/env python
"""DyGFormer past 128 tokens per pair: the native long route (TGMX_DYGFORMER_LONG=native: the one-call forward / backward with the streaming
attention of csrc/mha_stream.hip) against the composed path (TGMX_DYGFORMER_LONG=torch), at the example's widths (tools/bench_dygformer.py:
node 128, time 100, channel 50, two heads, two layers, out 172, wiki-shaped stream) with ``max_input_sequence_length`` --seq (default 256,
patch 1: T = 512 tokens per pair) and --pairs pairs a batch.  The sampler runs once per batch before the timing.  Per path:

  forward_us     ``encode_pairs`` on the positive pairs, eval mode, no gradients
  train_us       the same call in train mode (the example's dropout 0.1) under gradients, a linear loss, backward, an SGD step
  *_peak_mb      ``torch.cuda.max_memory_allocated`` over one such call / step, above what was allocated before it

Call rates through Python, not kernel times.  A timed window loops over the batch list until it lasts at least --window-s seconds and ends
in a synchronise; the two paths take turns in one process (a warm-up window each, then one window each, three rounds) and a figure is the
median of its three windows.  Also recorded: the largest difference between the two paths' eval outputs on the last batch, relative to
max(1, |composed|).  Prints one JSON line; --out appends it.
    python tools/bench_dygformer_long.py [--seq L] [--pairs P] [--out profiles/rNN_bench_dygformer_long.jsonl]"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import HookManager, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import DyGFormer  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seq', type=int, default=256, help='max_input_sequence_length (tokens per pair: 2 x seq)')
ap.add_argument('--pairs', type=int, default=200, help='pairs a batch')
ap.add_argument('--edges', type=int, default=4_000)
ap.add_argument('--batches', type=int, default=4, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
ap.add_argument('--paths', type=str, default='native,torch', help='which paths take part (a trace run names one)')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, dN, dT, C, E_, H, NL = args.pairs, args.seq - 1, 128, 100, 50, 172, 2, 2
s = make_stream('wiki', num_edges=args.edges)
N, dE = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
node_x = torch.randn(N, dN, device=dev)
hm = HookManager(keys=['k'])
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst'], ['edge_time', 'edge_time']))
with hm.activate('k'):
    batches = list(DGDataLoader(dg, batch_size=bs, hook_manager=hm))
work = [b for b in batches if b.edge_src.numel() == bs][-args.batches :]
torch.manual_seed(1)
w_loss = torch.randn(2, bs, E_, device=dev) / (2 * bs)
ar = torch.arange(bs, device=dev, dtype=torch.int32)
ENV = 'TGMX_DYGFORMER_LONG'
PATHS = [p for p in args.paths.split(',') if p]


def encode(enc, b):
    return enc.encode_pairs(node_x, b.edge_src, b.edge_dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], ar, ar + bs)


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * len(work)) * 1e6


def alternating_medians(fns):
    for fn in fns:
        window(fn)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / (window(fn) * len(work)))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(x, 1) for x in v] for v in seen]


def forward_runner(enc0, path):
    enc = copy.deepcopy(enc0).eval()

    def run(batches=work):
        os.environ[ENV] = path
        with torch.no_grad():
            outs = [encode(enc, b) for b in batches]
        os.environ.pop(ENV, None)
        return outs

    return run


def train_runner(enc0, path):
    enc = copy.deepcopy(enc0).train()
    opt = torch.optim.SGD([p for p in enc.parameters() if p.requires_grad], lr=1e-6)

    def run(batches=work):
        os.environ[ENV] = path
        for b in batches:
            opt.zero_grad(set_to_none=True)
            outs = encode(enc, b)
            assert ('DyGFormerFunction' in type(outs[0].grad_fn).__name__) == (path == 'native'), type(outs[0].grad_fn).__name__
            sum((o * w).sum() for o, w in zip(outs, w_loss)).backward()
            opt.step()
        os.environ.pop(ENV, None)

    return run


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(work[-1:])
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


torch.manual_seed(0)
enc0 = DyGFormer(node_feat_dim=dN, edge_x_dim=dE, time_feat_dim=dT, channel_embedding_dim=C, output_dim=E_, patch_size=1, num_layers=NL, num_heads=H,
                 dropout=0.1, max_input_sequence_length=K + 1, device=dev).to(dev)  # fmt: skip
line = {'bench': 'dygformer_long', 'device': torch.cuda.get_device_name(0), 'seq': args.seq, 'tokens_per_pair': 2 * args.seq, 'pairs': bs,
        'batches_timed': len(work), 'edge_dim': dE, 'node_dim': dN, 'time_dim': dT, 'channel_dim': C, 'heads': H, 'layers': NL, 'out_dim': E_,
        'what': 'encode_pairs on the positive pairs; train = dropout 0.1 + linear loss + backward + SGD step; call rates through Python'}  # fmt: skip
for kind, make in (('forward', forward_runner), ('train', train_runner)):
    fns = [make(enc0, p) for p in PATHS]
    med, seen = alternating_medians(fns)
    for p, m, v, fn in zip(PATHS, med, seen, fns):
        line[f'{kind}_us_{p}'], line[f'{kind}_windows_us_{p}'], line[f'{kind}_peak_mb_{p}'] = round(m, 1), v, peak_mb(fn)
    if kind == 'forward' and len(PATHS) == 2:
        a, b = (fn(work[-1:])[0] for fn in fns)
        line['forward_max_rel_diff'] = max(float(((x - y).abs() / y.abs().clamp(min=1.0)).max()) for x, y in zip(a, b))
if len(PATHS) == 2:
    line['native_is_faster_in_both'] = bool(line['forward_us_native'] < line['forward_us_torch'] and line['train_us_native'] < line['train_us_torch'])
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
