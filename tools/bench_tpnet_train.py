#!/usr/bin/env python
"""The encoder's share of a TPNet training step at the example's shape (examples/linkproppred/tpnet.py: wiki-shaped stream, bs 200, seeds
src | dst | neg, k = [32], node 128 / time 100 / edge 172 -> output 172, two mixer layers, three random-projection tables).  The sampler runs
once per batch before the timing; node_x carries no gradient, as in the example.  What is timed, per step, in microseconds -- a positive and
a negative TPNet.encode_pairs call under gradients in train mode, BCE on the pair logits, backward, an SGD step over all of
model.parameters() that train (so the packed copies of the weights the backward reads are rebuilt every step, as in real training):

  native  TGMX_TPNET_BWD=native: tgmx_tpnet_forward_train (the saving forward), tgmx_tpnet_backward as one call
  torch   TGMX_TPNET_BWD=torch: TPNet._torch_forward and autograd -- the training path as it was before the native one

with dropout = 0 and the example's dropout = 0.1, for concat and for cross pair features: four comparisons a run.  These are call rates
through Python (ctypes, autograd, the optimizer), not kernel times.  A timed window loops over the batch list until it lasts at least
--window-s seconds and ends in a synchronise; the two paths take turns in one process (one window each, three rounds, after a warm-up window
each) and each figure is the median of its three windows.  Also recorded, at dropout = 0: the largest relative difference between the two
paths' gradients (per parameter, against the gradient's largest entry) from the same weights on the last batch.  Prints one JSON line; --out
appends it.  --native-only N: N native steps and nothing else (for a kernel trace).
    python tools/bench_tpnet_train.py [--edges E] [--batches B] [--out profiles/rNN_bench_tpnet_train.jsonl]"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import RandomProjectionModule, TPNet  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=8_000)
ap.add_argument('--batches', type=int, default=8, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
ap.add_argument('--native-only', type=int, default=0, help='run this many native steps (concat, dropout 0.1) and exit')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, dN, dT, E_ = 200, 32, 128, 100, 172
s = make_stream('wiki', num_edges=args.edges)
N, D = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
node_x = torch.randn(N, dN, device=dev)
hm = HookManager(keys=['k'])
hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
with hm.activate('k'):
    batches = list(DGDataLoader(dg, batch_size=bs, hook_manager=hm))
warm = [b for b in batches if b.edge_src.numel() == bs]
work = warm[-args.batches :]  # steady state: full neighbour windows
ENV = 'TGMX_TPNET_BWD'
ar = torch.arange(bs, device=dev, dtype=torch.int32)


def model(concat: bool, p: float) -> TPNet:
    torch.manual_seed(0)
    rp = RandomProjectionModule(N, 2, 1e-6, 0, use_matrix=False, num_edges=110_000, dim_factor=10, concat_src_dst=concat)
    m = TPNet(dN, D, dT, E_, K, num_layers=2, dropout=p, random_projections=rp, device=dev).to(dev)
    for b in warm[: -args.batches]:  # the tables as they stand when the timed batches arrive
        rp.update(b.edge_src, b.edge_dst, b.edge_time)
    return m


def step_loss(m, b):
    """The example's step: positive and negative pairs through encode_pairs, BCE on the dot-product logits."""
    x = (node_x, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0])
    ps, pd = m.encode_pairs(x[0], b.edge_src, b.edge_dst, *x[1:], ar, ar + bs)
    ns, nd = m.encode_pairs(x[0], b.edge_src, b.neg, *x[1:], ar, ar + 2 * bs)
    pos, neg = (ps * pd).sum(1), (ns * nd).sum(1)
    return ps, F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))


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


def make_runner(m0, path):
    m = copy.deepcopy(m0).train()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-6)

    def run():
        os.environ[ENV] = path
        for b in work:
            opt.zero_grad(set_to_none=True)
            ps, loss = step_loss(m, b)
            assert (type(ps.grad_fn).__name__ == 'TPNetFunctionBackward') == (path == 'native'), type(ps.grad_fn).__name__
            loss.backward()
            opt.step()
        os.environ.pop(ENV, None)

    return run


def gradients(m0, path):
    """every parameter's gradient on the last batch, from the untrained weights"""
    m = copy.deepcopy(m0).train()
    os.environ[ENV] = path
    step_loss(m, work[-1])[1].backward()
    os.environ.pop(ENV, None)
    return {k: p.grad for k, p in m.named_parameters() if p.requires_grad}


if args.native_only:
    run = make_runner(model(True, 0.1), 'native')
    for _ in range(max(1, args.native_only // len(work))):
        run()
    torch.cuda.synchronize()
    sys.exit(0)

results, diffs = {}, {}
for concat in (True, False):
    for p in (0.0, 0.1):
        m0 = model(concat, p)
        (tn, tt), seen = alternating_medians([make_runner(m0, 'native'), make_runner(m0, 'torch')])
        key = f"{'concat' if concat else 'cross'}_dropout_{p:g}"
        results[key] = dict(native_us_per_step=round(tn, 1), torch_us_per_step=round(tt, 1), native_speedup=round(tt / tn, 2), native_is_faster=bool(tn < tt),
                            windows_us=seen)  # fmt: skip
        if p == 0.0:
            gn, gt = gradients(m0, 'native'), gradients(m0, 'torch')
            diffs[key] = max(float((gn[k] - gt[k]).abs().max()) / max(float(gt[k].abs().max()), 1e-30) for k in gn)
line = {
    'bench': 'tpnet_train_example', 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs, 'k': K,
    'edge_dim': D, 'time_dim': dT, 'node_dim': dN, 'output_dim': E_, 'num_layers': 2, 'tables': 3,
    'what': 'positive + negative encode_pairs + BCE + backward + SGD step, call rates through Python',
    **results, 'native_is_faster_in_all': bool(all(r['native_is_faster'] for r in results.values())),
    'native_vs_torch_max_rel_grad_diff': {k: float(f'{v:.3e}') for k, v in diffs.items()},
}  # fmt: skip
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
