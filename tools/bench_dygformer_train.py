#!/usr/bin/env python
"""The encoder's share of a DyGFormer training step at the example's shape (examples/linkproppred/dygformer.py; the workload of
tools/bench_dygformer.py: wiki-shaped stream, bs 200, k = [31] so L = 32, patch 1, channel 50, two heads, two layers, node 128, time 100,
out 172).  The sampler runs once per batch before the timing; node_x carries no gradient, as in the example.  What is timed, per step, in
microseconds -- the positive and the negative ``encode_pairs`` call under gradients in train mode, a linear loss on the four outputs,
backward, an SGD step (so the copies of the weights the backward reads, and their transposes, are rebuilt every step, as in real training):

  native  TGMX_DYGFORMER_BWD=native: tgmx_dygformer_forward_train (the saving forward), tgmx_dygformer_backward as one call
  py      TGMX_DYGFORMER_BWD=py: the same forward, the backward's launches one ctypes call each
  torch   TGMX_DYGFORMER_BWD=torch: DyGFormer._torch_forward and autograd -- the training path as it was before the native one

once with dropout = 0 and once with the example's dropout = 0.1.  These are call rates through Python (ctypes, autograd, the optimizer),
not kernel times.  A timed window loops over the batch list until it lasts at least --window-s seconds and ends in a synchronise; the three
paths take turns in one process (one window each, three rounds, after a warm-up window each) and each figure is the median of its three
windows.  Also recorded, at dropout = 0: the largest relative difference between the native and the composed path's gradients (per
parameter, against the gradient's largest entry) from the same weights on the last batch.  Prints one JSON line; --out appends it.
    python tools/bench_dygformer_train.py [--edges E] [--batches B] [--out profiles/rNN_bench_dygformer_train.jsonl]"""
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
from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import DyGFormer  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=12_000)
ap.add_argument('--batches', type=int, default=10, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
ap.add_argument('--paths', type=str, default='native,py,torch', help='which paths take part (a trace run names one)')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, dN, dT, C, E_, H, NL = 200, 31, 128, 100, 50, 172, 2, 2
s = make_stream('wiki', num_edges=args.edges)
N, dE = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
node_x = torch.randn(N, dN, device=dev)
hm = HookManager(keys=['k'])
hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
with hm.activate('k'):
    batches = list(DGDataLoader(dg, batch_size=bs, hook_manager=hm))
work = [b for b in batches if b.edge_src.numel() == bs][-args.batches :]  # steady state: full neighbour windows
torch.manual_seed(1)
w_loss = torch.randn(4, bs, E_, device=dev) / (4 * bs)
ar = torch.arange(bs, device=dev, dtype=torch.int32)
ROWS = {False: (ar, ar + bs), True: (ar, ar + 2 * bs)}
ENV = 'TGMX_DYGFORMER_BWD'
PATHS = [p for p in args.paths.split(',') if p]


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * len(work)) * 1e6


def alternating_medians(fns):
    """Warm each up (which also sizes its window), then one window each in turn, three rounds: drift of the device hits all alike."""
    for fn in fns:
        window(fn)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / (window(fn) * len(work)))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(x, 1) for x in v] for v in seen]


def loss_of(enc, b):
    outs = []
    for neg in (False, True):
        sr, dr = ROWS[neg]
        outs += enc.encode_pairs(node_x, b.edge_src, b.neg if neg else b.edge_dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr)
    return outs, sum((o * w).sum() for o, w in zip(outs, w_loss))


def make_runner(enc0, path):
    enc = copy.deepcopy(enc0).train()
    opt = torch.optim.SGD([p for p in enc.parameters() if p.requires_grad], lr=1e-6)

    def run():
        os.environ[ENV] = path
        for b in work:
            opt.zero_grad(set_to_none=True)
            outs, loss = loss_of(enc, b)
            assert ('DyGFormerFunction' in type(outs[0].grad_fn).__name__) == (path != 'torch'), type(outs[0].grad_fn).__name__
            loss.backward()
            opt.step()
        os.environ.pop(ENV, None)

    return run


def gradients(enc0, path):
    """every parameter's gradient on the last batch, from the untrained weights"""
    enc = copy.deepcopy(enc0).train()
    os.environ[ENV] = path
    loss_of(enc, work[-1])[1].backward()
    os.environ.pop(ENV, None)
    return {k: p.grad for k, p in enc.named_parameters() if p.requires_grad}


results, diff = {}, {}
for p in (0.0, 0.1):
    torch.manual_seed(0)
    enc0 = DyGFormer(node_feat_dim=dN, edge_x_dim=dE, time_feat_dim=dT, channel_embedding_dim=C, output_dim=E_, patch_size=1, num_layers=NL, num_heads=H,
                     dropout=p, max_input_sequence_length=K + 1, device=dev).to(dev)  # fmt: skip
    med, seen = alternating_medians([make_runner(enc0, path) for path in PATHS])
    r = {f'{path}_us_per_step': round(m, 1) for path, m in zip(PATHS, med)}
    if 'native_us_per_step' in r and 'torch_us_per_step' in r:
        r['native_speedup'] = round(r['torch_us_per_step'] / r['native_us_per_step'], 2)
        r['native_is_faster'] = bool(r['native_us_per_step'] < r['torch_us_per_step'])
    r['windows_us'] = dict(zip(PATHS, seen))
    results[p] = r
    if p == 0.0 and 'native' in PATHS and 'torch' in PATHS:
        gn, gt = gradients(enc0, 'native'), gradients(enc0, 'torch')
        diff = {k: float((gn[k] - gt[k]).abs().max()) / max(float(gt[k].abs().max()), 1e-30) for k in gn}
line = {
    'bench': 'dygformer_train_example_shape', 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs, 'k': K,
    'edge_dim': dE, 'node_dim': dN, 'time_dim': dT, 'channel_dim': C, 'heads': H, 'layers': NL, 'out_dim': E_,
    'what': 'positive + negative encode_pairs + linear loss + backward + SGD step, call rates through Python',
    'dropout_0': results[0.0], 'dropout_0.1': results[0.1],
    'native_is_faster_in_both': bool(results[0.0].get('native_is_faster') and results[0.1].get('native_is_faster')),
    'native_vs_torch_max_rel_grad_diff': max(diff.values()) if diff else None,
    'native_vs_torch_rel_grad_diff': {k: float(f'{v:.3e}') for k, v in diff.items()},
}  # fmt: skip
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
