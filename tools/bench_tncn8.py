#!/usr/bin/env python
"""NCNPredictor k = 8 (two-hop common neighbours) with time decay at the TNCN example's shape: tools/bench_tncn.py's pipeline (wiki-shaped
stream, bs 200, k = [10] neighbours, memory / embed / time dims 100, edge dim 172) run once per batch before the timing; what is timed is the
decoder alone, per batch, in microseconds, through Python:

  train_pair        the training-style pair of calls (one positive, one negative, B = 200 each): the native call (``tgmx_ncn8_forward``), and
                    the same arithmetic composed from torch ops on the device (``_torch_xs`` + the MLP, under no_grad)
  eval_onevsmany    the evaluation-style calls (one positive source against --candidates negatives + its destination, B = 21,
                    ``duplicate_targets='all'``, --positives of them per batch) through ONE prepared adjacency per batch, its build timed with
                    it: native, and composed

A timed window loops over the batch list until it lasts at least --window-s seconds; the two variants of a figure take turns (one window
each, three rounds, after a warm-up window each) and each figure is the median of its three windows.  Prints one JSON line.
    python tools/bench_tncn8.py [--edges E] [--batches B]"""
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
from tgm_amd.hooks import DeduplicationHook, HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import GraphAttentionEmbedding, IdentityMessage, LastAggregator, NCNPredictor, TGNMemory, sampled_edge_list  # noqa: E402
from tgm_amd.nn.ncn import adjacency  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=8_000)
ap.add_argument('--batches', type=int, default=10, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
ap.add_argument('--candidates', type=int, default=20, help='negatives per positive in the evaluation-style calls')
ap.add_argument('--positives', type=int, default=50, help='evaluation-style calls per batch')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, M, T_ = 200, 10, 100, 100
s = make_stream('wiki', num_edges=args.edges)
N, dE = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
hm = HookManager(keys=['k'])
hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
hm.register('k', DeduplicationHook(seed_nodes_keys=['neg', 'nbr_nids']))
torch.manual_seed(0)
mem = TGNMemory(N, dE, M, T_, IdentityMessage(dE, M, T_), LastAggregator()).to(dev).train()
enc = GraphAttentionEmbedding(M, 100, dE, mem.time_enc).to(dev).eval()

work = []  # per batch: the decoder's inputs, cloned out of the pipeline's pooled buffers
with hm.activate('k'), torch.no_grad():
    for batch in DGDataLoader(dg, batch_size=bs, hook_manager=hm):
        if batch.edge_src.numel() == bs:
            ei, et, ex = sampled_edge_list(batch)
            z, lu = mem(batch.unique_nids)
            z = enc(z, lu, ei, et, ex)
            loc = lambda ids: batch.global_to_local(ids).long()
            src, dst, neg = loc(batch.edge_src), loc(batch.edge_dst), loc(batch.neg)
            buf = torch.empty((2, ei.shape[1] + 64), dtype=torch.int64, device=dev)  # a strided view, as sampled_edge_list hands it out
            buf[:, : ei.shape[1]] = ei
            work.append(dict(z=z.clone(), lu=lu.clone(), ei=buf[:, : ei.shape[1]], t=batch.edge_time.clone(), pos=torch.stack([src, dst]),
                             neg=torch.stack([src, neg]),
                             many=[torch.stack([src[p].repeat(args.candidates + 1), torch.cat([dst[p : p + 1], neg[: args.candidates]])]) for p in range(args.positives)],
                             many_t=[batch.edge_time[p].repeat(args.candidates + 1) for p in range(args.positives)]))  # fmt: skip
        mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_x)
work = work[-args.batches :]  # steady state: full neighbour windows


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


def composed(m, z, ei, tar, lu, t):
    return m.xsmlp(m._torch_xs(m._inputs(z, ei, tar, lu, t))).view(-1)


torch.manual_seed(8)
dec = NCNPredictor(100, 100, 1, k=8, cn_time_decay=True).to(dev).eval()
dec_all = NCNPredictor(100, 100, 1, k=8, cn_time_decay=True, duplicate_targets='all').to(dev).eval()
dec_all.load_state_dict(dec.state_dict())


def train_native():
    for w in work:
        dec(w['z'], w['ei'], w['pos'], w['lu'], w['t'])
        dec(w['z'], w['ei'], w['neg'], w['lu'], w['t'])


def train_composed():
    for w in work:
        composed(dec, w['z'], w['ei'], w['pos'], w['lu'], w['t'])
        composed(dec, w['z'], w['ei'], w['neg'], w['lu'], w['t'])


def eval_native():
    for w in work:
        adj = adjacency(w['z'].shape[0], w['ei'])
        for tar, t in zip(w['many'], w['many_t']):
            dec_all(w['z'], adj, tar, w['lu'], t)


def eval_composed():
    for w in work:
        adj = adjacency(w['z'].shape[0], w['ei'])
        for tar, t in zip(w['many'], w['many_t']):
            composed(dec_all, w['z'], adj, tar, w['lu'], t)


with torch.no_grad():
    (tn, tc), train_seen = alternating_medians([train_native, train_composed])
    (en, ec), eval_seen = alternating_medians([eval_native, eval_composed])
    w = work[-1]
    a, c = dec(w['z'], w['ei'], w['neg'], w['lu'], w['t']), composed(dec, w['z'], w['ei'], w['neg'], w['lu'], w['t'])
    agree = float(((a - c).abs() / c.abs().clamp(min=1)).max())
    active = float(dec.get_cn_emb(w['z'], w['ei'], w['pos'], (w['lu'], w['t'])).any(dim=1).float().mean())
print(json.dumps({
    'bench': 'tncn8_decoder_example_shape', 'k': 8, 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs,
    'sampled_edges_per_batch': round(statistics.mean(w['ei'].shape[1] for w in work)), 'local_nodes_per_batch': round(statistics.mean(w['z'].shape[0] for w in work)),
    'candidates': args.candidates, 'positives_per_batch': args.positives, 'pairs_with_a_block_in_the_last_positive_call': round(active, 3),
    'train_pair_native_us_per_batch': round(tn, 1), 'train_pair_composed_us_per_batch': round(tc, 1), 'train_pair_native_speedup': round(tc / tn, 2),
    'eval_native_us_per_batch': round(en, 1), 'eval_composed_us_per_batch': round(ec, 1), 'eval_native_speedup': round(ec / en, 2),
    'train_windows_us': train_seen, 'eval_windows_us': eval_seen, 'native_vs_composed_max_rel_diff': agree,
}), flush=True)  # fmt: skip
