#!/usr/bin/env python
"""The encoder's share of a CTAN training step at the example's shape (examples/linkproppred/ctan.py; the workload of tools/bench_ctan.py:
wiki-shaped stream, bs 200, seeds src | dst | neg, num_nbrs = [32], memory = time dim 256, edge dim 172, node dim 1, 3 iterations, epsilon
0.5, gamma 0.1).  The sampler, DeduplicationHook and ``sampled_edge_list`` run once per batch before the timing and the memory is rolled
forward with the native modules; node_x carries no gradient (the memory is a buffer), as in the example.  What is timed, per step, in
microseconds -- CTAN.forward under gradients, a linear loss on its output, backward, an SGD step (so the stacked weights and their
transposes are rebuilt every step, as in real training):

  native  the native training path: tgmx_ctan_forward in its saving form, tgmx_ctan_backward as one call
  torch   TGMX_CTAN_BWD=torch: CTAN.forward_composed and autograd -- the training path as it was before the native one, unchanged

These are call rates through Python (ctypes, autograd, the optimizer), not kernel times.  A timed window loops over the batch list until it
lasts at least --window-s seconds and ends in a synchronise; the two paths take turns in one process (one window each, three rounds, after a
warm-up window each) and each figure is the median of its three windows.  Also recorded: the largest relative difference between the two
paths' gradients (per parameter, against the gradient's largest entry) from the same weights on the last batch.  Prints one JSON line;
--out appends it.
    python tools/bench_ctan_train.py [--edges E] [--batches B] [--out profiles/rNN_bench_ctan_train.jsonl]"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import DeduplicationHook, HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import sampled_edge_list  # noqa: E402
from tgm_amd.nn.encoder import CTAN, CTANMemory, LastAggregator  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=12_000)
ap.add_argument('--batches', type=int, default=10, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, M, T_, ITERS = 200, 32, 256, 256, 3
s = make_stream('wiki', num_edges=args.edges)
N, dE = s.num_nodes, s.edge_x.shape[1]


def delta_t_stats(src, dst, ts, start):
    """compute_delta_t_stats of the example"""
    last, deltas = {}, []
    for a, b, t in zip(src.tolist(), dst.tolist(), ts.tolist()):
        deltas.extend([t - last.get(a, start), t - last.get(b, start)])
        last[a] = last[b] = t
    return float(np.mean(deltas)), float(np.std(deltas))


mean_dt, std_dt = delta_t_stats(s.src, s.dst, s.ts, int(s.ts[0]))
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
hm = HookManager(keys=['k'])
hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
hm.register('k', DeduplicationHook(seed_nodes_keys=['neg', 'nbr_nids']))
torch.manual_seed(0)
mem = CTANMemory(N, M, aggr_module=LastAggregator(), init_time=int(s.ts[0])).to(dev).eval()
enc0 = CTAN(edge_dim=dE, memory_dim=M, time_dim=T_, node_dim=1, num_iters=ITERS, mean_delta_t=mean_dt, std_delta_t=std_dt, epsilon=0.5, gamma=0.1).to(dev)
static_x = torch.randn(N, 1, device=dev)

work = []  # per batch: the encoder's inputs, cloned out of the pipeline's pooled buffers
with hm.activate('k'), torch.no_grad():
    for batch in DGDataLoader(dg, batch_size=bs, hook_manager=hm):
        ei, et, ex = sampled_edge_list(batch)
        uniq = batch.unique_nids.long()
        z0, lu = mem(uniq)
        x = torch.cat([z0, static_x[uniq]], dim=-1)
        z = enc0(x, lu, ei, et, ex)
        inv_src, inv_dst = batch.global_to_local(batch.edge_src).long(), batch.global_to_local(batch.edge_dst).long()
        if batch.edge_src.numel() == bs:
            work.append(dict(x=x.clone(), lu=lu.clone(), ei=ei.clone(), et=et.clone(), ex=ex.float().clone()))
        mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, z[inv_src], z[inv_dst])
work = work[-args.batches :]  # steady state: full neighbour windows
mem.check()
enc0.check()
torch.manual_seed(1)
for w in work:
    w['w_loss'] = torch.randn(w['x'].shape[0], M, device=dev) / w['x'].shape[0]


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


def set_path(path):
    if path == 'torch':
        os.environ['TGMX_CTAN_BWD'] = 'torch'
    else:
        os.environ.pop('TGMX_CTAN_BWD', None)


def make_runner(path):
    enc = copy.deepcopy(enc0).train()
    opt = torch.optim.SGD(enc.parameters(), lr=1e-6)
    want = 'Ctan' if path == 'native' else 'Tanh'

    def run():
        set_path(path)
        for w in work:
            opt.zero_grad(set_to_none=True)
            out = enc(w['x'], w['lu'], w['ei'], w['et'], w['ex'])
            assert want in type(out.grad_fn).__name__, type(out.grad_fn).__name__
            (out * w['w_loss']).sum().backward()
            opt.step()
        os.environ.pop('TGMX_CTAN_BWD', None)

    return run, enc


def gradients(path):
    """every parameter's gradient on the last batch, from the untrained weights"""
    enc = copy.deepcopy(enc0).train()
    set_path(path)
    w = work[-1]
    (enc(w['x'], w['lu'], w['ei'], w['et'], w['ex']) * w['w_loss']).sum().backward()
    os.environ.pop('TGMX_CTAN_BWD', None)
    enc.check()
    return {k: p.grad for k, p in enc.named_parameters()}


(native, enc_n), (composed, enc_t) = make_runner('native'), make_runner('torch')
(tn, tt), seen = alternating_medians([native, composed])
enc_n.check()
enc_t.check()
gn, gt = gradients('native'), gradients('torch')
diff = {}
for k in gn:
    scale = float(gt[k].abs().max())
    if k == 'aconv.phi.lin_key.bias':  # its exact gradient is 0: the scale of the terms that cancel in it
        scale = float(gt['aconv.phi.lin_query.bias'].abs().max())
    diff[k] = float((gn[k] - gt[k]).abs().max()) / max(scale, 1e-30)
line = {
    'bench': 'ctan_train_example_shape', 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs, 'num_nbrs': K,
    'memory_dim': M, 'time_dim': T_, 'edge_dim': dE, 'num_iters': ITERS,
    'sampled_edges_per_batch': round(statistics.mean(w['ei'].shape[1] for w in work)), 'local_nodes_per_batch': round(statistics.mean(w['x'].shape[0] for w in work)),
    'what': 'encoder forward + linear loss + backward + SGD step, call rates through Python',
    'native_us_per_step': round(tn, 1), 'torch_us_per_step': round(tt, 1), 'native_speedup': round(tt / tn, 2), 'native_is_faster': bool(tn < tt),
    'windows_us': seen, 'native_vs_torch_max_rel_grad_diff': max(diff.values()), 'native_vs_torch_rel_grad_diff': {k: float(f'{v:.3e}') for k, v in diff.items()},
}  # fmt: skip
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
