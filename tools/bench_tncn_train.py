#!/usr/bin/env python
"""The decoder's share of a TNCN training step at the example's shape (examples/linkproppred/tncn.py's train(): a wiki-shaped stream, batch
size 200, one hop of 10 neighbours, every width 100, time decay on): ``NCNPredictor`` on the positives and on the negatives, BCE with
logits, and the backward down to ``z.grad`` and the parameters' gradients.  Per step, in microseconds, for k = 2 and k = 4:

  native  tgmx_ncn_forward twice (activations kept by each call), tgmx_ncn_backward twice
  torch   TGMX_NCN_BWD=torch: the composed torch path through dense [B, N] rows, what the decoder did before it had a backward

The decoder's inputs -- z, the sampled edge list, the local targets, last_update -- come from the last full batch of the stream, through
the sampler, TGNMemory and GraphAttentionEmbedding (not timed).  Every step ends with an optimizer step (SGD; both variants pay it) so
that whatever a variant caches against the parameters' versions is rebuilt once per step, inside the timing.  A timed window repeats the
step until it lasts at least --window-s seconds; the variants take turns (one window each, three rounds, after a warm-up window each) and
each figure is the median of its three windows; the whole schedule runs twice (``runs``).  These are call rates through Python: the
launches themselves are not traced.  Prints one JSON line; --out appends it.
    python tools/bench_tncn_train.py [--out profiles/rNN_bench_tncn_train.jsonl]"""
import argparse
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
from tgm_amd.hooks import DeduplicationHook, HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import GraphAttentionEmbedding, IdentityMessage, LastAggregator, NCNPredictor, TGNMemory, sampled_edge_list  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--window-s', type=float, default=0.15, help='least duration of a timed window')
ap.add_argument('--edges', type=int, default=8_000, help='length of the stream; the last full batch is timed')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()
dev = torch.device('cuda', 0)
B, DIM = 200, 100


def decoder_inputs():
    """(z, edge_index, positive targets, negative targets, last_update, edge_time) of the last full batch of the stream: steady state, full
    neighbour windows (tools/bench_tncn.py's pipeline)"""
    torch.manual_seed(0)
    s = make_stream('wiki', num_edges=args.edges)
    N, dE = s.num_nodes, s.edge_x.shape[1]
    dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
    hm.register('k', RecencyNeighborHook(N, [10], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    hm.register('k', DeduplicationHook(seed_nodes_keys=['neg', 'nbr_nids']))
    mem = TGNMemory(N, dE, DIM, DIM, IdentityMessage(dE, DIM, DIM), LastAggregator()).to(dev).train()
    enc = GraphAttentionEmbedding(DIM, DIM, dE, mem.time_enc).to(dev).eval()
    kept = None
    with hm.activate('k'), torch.no_grad():
        for batch in DGDataLoader(dg, batch_size=B, hook_manager=hm):
            if batch.edge_src.numel() == B:
                ei, et, ex = sampled_edge_list(batch)
                z, lu = mem(batch.unique_nids)
                z = enc(z, lu, ei, et, ex)
                loc = lambda ids: batch.global_to_local(ids).long()
                pos = torch.stack([loc(batch.edge_src), loc(batch.edge_dst)])
                neg = torch.stack([loc(batch.edge_src), loc(batch.neg)])
                kept = (z.clone(), ei.clone(), pos, neg, lu.clone(), batch.edge_time.clone())
            mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_x)
    return kept


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def alternating_medians(fns):
    for fn in fns:
        window(fn, 3)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / window(fn, 5))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(v, 1) for v in vs] for vs in seen]


def with_env(value, fn):
    def run():
        if value is None:
            os.environ.pop('TGMX_NCN_BWD', None)
        else:
            os.environ['TGMX_NCN_BWD'] = value
        try:
            return fn()
        finally:
            os.environ.pop('TGMX_NCN_BWD', None)

    return run


z0, ei, pos_t, neg_t, lu, et = decoder_inputs()
line = {'bench': 'tncn_train_example_shape', 'device': torch.cuda.get_device_name(0), 'batch_size': B, 'local_nodes': z0.shape[0],
        'sampled_edges': ei.shape[1], 'runs': []}  # fmt: skip
ones, zeros = torch.ones(B, device=dev), torch.zeros(B, device=dev)
for run in range(2):
    res = {}
    for k in (2, 4):
        torch.manual_seed(k)
        dec = NCNPredictor(DIM, DIM, 1, k=k, cn_time_decay=True).to(dev).train()
        opt = torch.optim.SGD(dec.parameters(), lr=1e-3)
        grads = {}

        def step(tag):
            z = z0.detach().requires_grad_()
            opt.zero_grad(set_to_none=True)
            loss = F.binary_cross_entropy_with_logits(dec(z, ei, pos_t, lu, et), ones) + F.binary_cross_entropy_with_logits(dec(z, ei, neg_t, lu, et), zeros)
            loss.backward()
            grads[tag] = [z.grad] + [p.grad for p in dec.xsmlp.parameters()]
            opt.step()

        fns = [with_env(None, lambda: step('native')), with_env('torch', lambda: step('torch'))]
        # the two variants' gradients on the same, freshly drawn parameters (lr = 0: these steps change nothing)
        for group in opt.param_groups:
            group['lr'] = 0.0
        for fn in fns:
            fn()
        rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1)).max())
        res[f'k{k}_max_rel_diff'] = max(rel(a, t) for a, t in zip(grads['native'], grads['torch']))
        for group in opt.param_groups:
            group['lr'] = 1e-3
        med, seen = alternating_medians(fns)
        res.update({f'k{k}_{n}_us': round(t, 1) for n, t in zip(('native', 'torch'), med)})
        res[f'k{k}_windows_us'] = seen
        res[f'k{k}_speedup'] = round(med[1] / med[0], 2)
    line['runs'].append(res)
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
