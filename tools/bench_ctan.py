#!/usr/bin/env python
"""CTAN at the example's shape (examples/linkproppred/ctan.py: wiki-shaped stream, bs 200, seeds src | dst | neg, num_nbrs = [32], memory =
time dim 256, edge dim 172, node dim 1, 3 iterations, epsilon 0.5, gamma 0.1, mean / std of the time gaps computed from the stream as
the example does).  The sampler, DeduplicationHook and ``sampled_edge_list`` run once per batch before the timing, the memory is rolled
forward with the native modules; what is timed, per batch, in microseconds:

  forward        CTAN.forward under no_grad: the native call (tgmx_ctan_forward) against the same forward composed from torch ops on the
                 device (CTAN.forward_composed)
  update_state   CTANMemory.update_state: native (tgmx_ctan_memory_update) against the reference's unique + score-matrix composition
                 on the device
  attend         the new attention launch (tgmx_ctan_attend, mode 0) against tgmx_tconv_attend -- the generic walk of the same library -- on
                 identical inputs at H = 1, C = 256: the batch's q, k, v, edge projection and segments

A timed window loops over the batch list until it lasts at least --window-s seconds; the variants of one figure take turns (one window
each, three rounds, after a warm-up window each) and each figure is the median of its three windows.  Prints one JSON line; --out
appends it to a file.
    python tools/bench_ctan.py [--edges E] [--batches B] [--out profiles/rNN_bench_ctan.jsonl]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph, _native  # noqa: E402
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
enc = CTAN(edge_dim=dE, memory_dim=M, time_dim=T_, node_dim=1, num_iters=ITERS, mean_delta_t=mean_dt, std_delta_t=std_dt, epsilon=0.5, gamma=0.1).to(dev).eval()
static_x = torch.randn(N, 1, device=dev)
lib = _native.load()

work = []  # per batch: the model's inputs, cloned out of the pipeline's pooled buffers
with hm.activate('k'), torch.no_grad():
    for batch in DGDataLoader(dg, batch_size=bs, hook_manager=hm):
        ei, et, ex = sampled_edge_list(batch)
        uniq = batch.unique_nids.long()
        z0, lu = mem(uniq)
        x = torch.cat([z0, static_x[uniq]], dim=-1)
        z = enc(x, lu, ei, et, ex)
        inv_src, inv_dst = batch.global_to_local(batch.edge_src).long(), batch.global_to_local(batch.edge_dst).long()
        if batch.edge_src.numel() == bs:
            work.append(dict(x=x.clone(), lu=lu.clone(), ei=ei.clone(), et=et.clone(), ex=ex.clone(), src=batch.edge_src.clone(), dst=batch.edge_dst.clone(),
                             t=batch.edge_time.clone(), se=z[inv_src].clone(), de=z[inv_dst].clone()))  # fmt: skip
        mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, z[inv_src], z[inv_dst])
work = work[-args.batches :]  # steady state: full neighbour windows
mem.check()
enc.check()

# the attention launch's inputs of every batch: first-iteration q, k, v and the edge projection, as the native forward computes them
phi = enc.aconv.phi
with torch.no_grad():
    for w in work:
        src, tgt = w['ei'][0].contiguous(), w['ei'][1].contiguous()
        rel = (((w['lu'][src] - w['et']).abs() - mean_dt) / std_dt).float()
        e = phi.lin_edge(torch.cat([w['ex'].float(), enc.time_enc(rel)], dim=-1)).contiguous()
        x0 = enc.enc_x(w['x'])
        order = torch.argsort(tgt, stable=True)
        U = x0.shape[0]
        ar = torch.arange(U, device=dev)
        w['att'] = dict(q=phi.lin_query(x0).contiguous(), k=phi.lin_key(x0).contiguous(), v=phi.lin_value(x0).contiguous(), e=e, order=order, src=src,
                        lo=torch.searchsorted(tgt[order], ar).contiguous(), hi=torch.searchsorted(tgt[order], ar, right=True).contiguous(), U=U,
                        out=torch.zeros(U, M, device=dev))  # fmt: skip


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


def fwd_native():
    for w in work:
        enc(w['x'], w['lu'], w['ei'], w['et'], w['ex'])


def fwd_composed():
    for w in work:
        enc.forward_composed(w['x'], w['lu'], w['ei'], w['et'], w['ex'])


def upd_native():
    for w in work:
        mem.update_state(w['src'], w['dst'], w['t'], w['se'], w['de'])


def upd_composed():
    for w in work:
        mem._update_state_composed(w['src'], w['dst'], w['t'], w['se'], w['de'], last=True)


def attend(new: bool):
    st = _native.stream_ptr()
    for w in work:
        a = w['att']
        common = (a['q'].data_ptr(), a['k'].data_ptr(), a['v'].data_ptr(), a['e'].data_ptr(), a['order'].data_ptr(), a['src'].data_ptr(),
                  a['lo'].data_ptr(), a['hi'].data_ptr(), a['U'])  # fmt: skip
        if new:
            _native.check(lib.tgmx_ctan_attend(*common, M, M**-0.5, a['out'].data_ptr(), None, None, 0.0, 0, st), 'tgmx_ctan_attend')
        else:
            _native.check(lib.tgmx_tconv_attend(*common, 1, M, M**-0.5, a['out'].data_ptr(), None, st), 'tgmx_tconv_attend')


with torch.no_grad():
    (fn_, fc), fwd_seen = alternating_medians([fwd_native, fwd_composed])
    (un, uc), upd_seen = alternating_medians([upd_native, upd_composed])
    (an, ag), att_seen = alternating_medians([lambda: attend(True), lambda: attend(False)])
    w = work[-1]
    a, c = enc(w['x'], w['lu'], w['ei'], w['et'], w['ex']), enc.forward_composed(w['x'], w['lu'], w['ei'], w['et'], w['ex'])
    agree = float(((a - c).abs() / c.abs().clamp(min=1)).max())
seg = torch.cat([w['att']['hi'] - w['att']['lo'] for w in work])
line = {
    'bench': 'ctan_example_shape', 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'batches_timed': len(work), 'bs': bs, 'num_nbrs': K,
    'memory_dim': M, 'time_dim': T_, 'edge_dim': dE, 'num_iters': ITERS, 'mean_delta_t': round(mean_dt, 1), 'std_delta_t': round(std_dt, 1),
    'sampled_edges_per_batch': round(statistics.mean(w['ei'].shape[1] for w in work)), 'local_nodes_per_batch': round(statistics.mean(w['x'].shape[0] for w in work)),
    'longest_segment': int(seg.max()), 'segments_over_16': int((seg > 16).sum()) // len(work),
    'forward_native_us_per_batch': round(fn_, 1), 'forward_composed_us_per_batch': round(fc, 1), 'forward_native_speedup': round(fc / fn_, 2),
    'update_state_native_us_per_batch': round(un, 1), 'update_state_composed_us_per_batch': round(uc, 1), 'update_state_native_speedup': round(uc / un, 2),
    'attend_new_us_per_batch': round(an, 1), 'attend_generic_us_per_batch': round(ag, 1), 'attend_new_speedup': round(ag / an, 2),
    'forward_windows_us': fwd_seen, 'update_state_windows_us': upd_seen, 'attend_windows_us': att_seen, 'native_vs_composed_max_rel_diff': agree,
}  # fmt: skip
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
