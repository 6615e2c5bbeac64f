#!/usr/bin/env python
"""The Base3 ensemble (EdgeBankPredictor averaged with tCoMemPredictor) at the example's shape: a wiki-shaped stream, both memories loaded
with its first 70 %, then evaluation batches of bs = 200 positives with 999 negatives each (200 000 queries a batch) followed by the batch's
updates, k = 50.  Two runs: queries handed over as int64 ids (what the example does: the co-occurrence term is truncated to 0) and as float32
ids (the term is added).  Per batch, in microseconds:

  tcomem_query_200_calls     the example's loop: one t-CoMem call per positive edge (1 000 queries each), inputs built beforehand
  tcomem_query_one_vs_many   the same answers from one ``query_one_vs_many`` call
  tcomem_update              ``update`` with the batch's 200 edges
  base3_step                 both predictors' one-against-many queries, their average, and both updates

each measured three ways in the same process:

  native     tgm_amd.nn.tCoMemPredictor (csrc/tcomem.hip) and tgm_amd.nn.EdgeBankPredictor (csrc/edgebank.hip)
  composed   the same from torch ops on the device: the ring arithmetic vectorised over [B, k], the ring update through a stable sort, the
             pair counts and EdgeBank's memory as sorted packed keys behind ``searchsorted``
  host       the reference's algorithms on the host (tests/tcomem_restate.py, tests/edgebank_restate.py), on a few batches, once

A timed window loops over the batch list until it lasts at least --window-s seconds; the variants of one figure take turns (one window
each, three rounds, after a warm-up window each) and each figure is the median of its three windows.  The timed loops offer the same
batches again and again; the predictors' counts of offered events are put back after every pass, so that the tables keep the size the
stream gives them.  Prints one JSON line per run.
    python tools/bench_base3.py [--edges E] [--batches B]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import edgebank_restate as er  # noqa: E402
import tcomem_restate as tr  # noqa: E402
from tgm_amd.nn import EdgeBankPredictor, tCoMemPredictor  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=157_474)
ap.add_argument('--batches', type=int, default=20, help='distinct batches a timed window loops over')
ap.add_argument('--host-batches', type=int, default=2, help='batches the host restatements are timed on')
ap.add_argument('--window-s', type=float, default=0.3, help='least duration of a timed window')
ap.add_argument('--negatives', type=int, default=999)
ap.add_argument('--k', type=int, default=50)
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, M, K, WEIGHT = 200, args.negatives, args.k, 0.8
s = make_stream('wiki', num_edges=args.edges, edge_dim=0)
N = int(s.num_nodes)
n_load = int(0.7 * args.edges)
src, dst, ts = s.src.to(dev).long(), s.dst.to(dev).long(), s.ts.to(dev).long()
n_src = int(s.src.max()) + 1
gen = torch.Generator().manual_seed(11)
batches = []
for b in range(args.batches):
    lo = n_load + b * bs
    neg = torch.randint(n_src, N, (bs, M), generator=gen, dtype=torch.int64).to(dev)  # destinations of the bipartite stream
    batches.append(dict(src=src[lo : lo + bs], dst=dst[lo : lo + bs], ts=ts[lo : lo + bs], neg=neg))


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * len(batches)) * 1e6


def alternating_medians(fns):
    for fn in fns:
        window(fn)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / (window(fn) * len(batches)))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(x, 1) for x in v] for v in seen]


class ComposedEdgeBank:
    """EdgeBank (unlimited) from torch ops on the device: sorted packed keys and their timestamps"""

    def __init__(self, src, dst, ts):
        self.end, self.size = ts.max(), ts.max() - ts.min()
        self.keys = torch.empty(0, dtype=torch.int64, device=dev)
        self.update(src, dst, ts)

    def update(self, src, dst, ts):
        self.end = torch.max(self.end, ts.max())
        ok = ts >= self.end - self.size
        self.keys = torch.unique(torch.cat([self.keys, (src << 32 | dst)[ok]]))  # sorted; unlimited mode never looks at the timestamp again

    def one_vs_many(self, src, dst, neg):
        q = src[:, None] << 32 | torch.cat([dst[:, None], neg], 1)
        i = torch.searchsorted(self.keys, q).clamp_(max=self.keys.numel() - 1)
        return (self.keys[i] == q).to(src.dtype)


class ComposedTCoMem:
    """t-CoMem from torch ops on the device"""

    def __init__(self, src, dst, ts):
        self.end = ts.max()
        self.size = torch.clamp(ts.max() - ts.min(), min=1.0)
        self.recent_ts = torch.full((N, K), -float('inf'), device=dev)
        self.recent_dst = torch.zeros((N, K), dtype=torch.int64, device=dev)
        self.pos = torch.zeros(N, dtype=torch.int64, device=dev)
        self.len = torch.zeros(N, dtype=torch.int64, device=dev)
        self.pop = torch.zeros(N, device=dev)
        self.keys = torch.empty(0, dtype=torch.int64, device=dev)
        self.counts = torch.empty(0, dtype=torch.int64, device=dev)
        for lo in range(0, len(src), 1 << 16):
            self.update(src[lo : lo + (1 << 16)], dst[lo : lo + (1 << 16)], ts[lo : lo + (1 << 16)])

    def update(self, src, dst, ts):
        n = len(src)
        self.end = torch.max(self.end, ts.max())
        # the ring: rank of every event among its source's events of this call (arrival order) and their number
        ssrc, order = torch.sort(src, stable=True)
        idx = torch.arange(n, device=dev)
        first = torch.ones(n, dtype=torch.bool, device=dev)
        first[1:] = ssrc[1:] != ssrc[:-1]
        start = torch.cummax(torch.where(first, idx, 0), 0).values
        last = torch.ones(n, dtype=torch.bool, device=dev)
        last[:-1] = first[1:]
        end = torch.flip(torch.cummin(torch.flip(torch.where(last, idx, n), [0]), 0).values, [0])
        rank, cnt = idx - start, end - start + 1
        pos0 = self.pos[ssrc]
        keep = rank >= cnt - K
        flat = ssrc * K + (pos0 + rank) % K
        self.recent_ts.view(-1)[flat[keep]] = ts[order][keep].float()
        self.recent_dst.view(-1)[flat[keep]] = dst[order][keep]
        self.pos[ssrc[last]] = ((pos0 + cnt) % K)[last]
        self.len[ssrc[last]] = torch.clamp(self.len[ssrc[last]] + cnt[last], max=K)
        self.pop.index_add_(0, dst, torch.ones(n, device=dev))
        # the pair counts: sorted keys, equal keys summed
        keys = torch.cat([self.keys, torch.minimum(src, dst) << 32 | torch.maximum(src, dst)])
        add = torch.cat([self.counts, torch.where(src == dst, 2, 1)])
        self.keys, inv = torch.unique(keys, return_inverse=True)
        self.counts = torch.zeros(len(self.keys), dtype=torch.int64, device=dev).index_add_(0, inv, add)

    def base(self, src):
        endf = self.end.float()
        start = endf - self.size
        t = self.recent_ts[src]
        mask = (torch.arange(K, device=dev)[None] < self.len[src][:, None]) & (t >= start) & (t <= endf)
        decay = torch.exp(-(endf - torch.where(mask, t, -float('inf'))) / self.size)
        return (decay * torch.sigmoid(self.pop[self.recent_dst[src]]) * mask).sum(1)

    def query(self, src, dst, with_term):
        base = self.base(src)
        if not with_term:
            return base
        return base + self._term(src, dst)

    def _term(self, src, dst):
        q = torch.minimum(src, dst) << 32 | torch.maximum(src, dst)
        i = torch.searchsorted(self.keys, q).clamp_(max=self.keys.numel() - 1)
        c = torch.where(self.keys[i] == q, self.counts[i], 0).double()
        return (WEIGHT * (c / (1 + c))).float()

    def one_vs_many(self, src, dst, neg, with_term):
        base = self.base(src)[:, None].expand(-1, neg.shape[1] + 1)
        if not with_term:
            return base.contiguous()
        return base + self._term(src[:, None].expand(-1, neg.shape[1] + 1), torch.cat([dst[:, None], neg], 1))


def run(query_dtype: str) -> dict:
    with_term = query_dtype == 'float32'
    qt = torch.float32 if with_term else torch.int64
    work = []
    for w in batches:
        q = dict(src=w['src'].to(qt), dst=w['dst'].to(qt), neg=w['neg'].to(qt))
        q['calls'] = [(q['src'][p].repeat(M + 1), torch.cat([q['dst'][p : p + 1], q['neg'][p]])) for p in range(bs)]
        work.append((w, q))
    bank = EdgeBankPredictor(src[:n_load], dst[:n_load], ts[:n_load])
    comem = tCoMemPredictor(src[:n_load], dst[:n_load], ts[:n_load], N, K, co_occurrence_weight=WEIGHT)
    c_bank = ComposedEdgeBank(src[:n_load], dst[:n_load], ts[:n_load])
    c_comem = ComposedTCoMem(src[:n_load], dst[:n_load], ts[:n_load])
    offered = [0, 0]

    def keep_size():  # (see the module docstring)
        bank._offered, comem._offered = offered

    def n_calls():
        for _, q in work:
            for qs, qd in q['calls']:
                comem(qs, qd)

    def n_many():
        for _, q in work:
            comem.query_one_vs_many(q['src'], q['dst'], q['neg'])

    def n_update():
        for w, _ in work:
            comem.update(w['src'], w['dst'], w['ts'])
        keep_size()

    def n_step():
        for w, q in work:
            a = bank.query_one_vs_many(q['src'], q['dst'], q['neg'])
            b = comem.query_one_vs_many(q['src'], q['dst'], q['neg'])
            (a + b) / 2
            bank.update(w['src'], w['dst'], w['ts'])
            comem.update(w['src'], w['dst'], w['ts'])
        keep_size()

    def c_calls():
        for w, q in work:
            for qs, qd in q['calls']:
                c_comem.query(qs.long(), qd.long(), with_term)

    def c_many():
        for w, _ in work:
            c_comem.one_vs_many(w['src'], w['dst'], w['neg'], with_term)

    def c_update():
        for w, _ in work:
            c_comem.update(w['src'], w['dst'], w['ts'])

    def c_step():
        for w, _ in work:
            a = c_bank.one_vs_many(w['src'], w['dst'], w['neg']).to(qt)
            b = c_comem.one_vs_many(w['src'], w['dst'], w['neg'], with_term)
            (a + b) / 2
            c_bank.update(w['src'], w['dst'], w['ts'])
            c_comem.update(w['src'], w['dst'], w['ts'])

    # agreement first, on the state the stream gives: every batch queried, then offered; three ways for the first host batches
    cpu = lambda t: t.cpu().numpy()
    h_bank = er.EdgeBankRestated(cpu(src[:n_load]), cpu(dst[:n_load]), cpu(ts[:n_load]))
    t0 = time.perf_counter()
    h_comem = tr.TCoMemRestated(cpu(src[:n_load]), cpu(dst[:n_load]), cpu(ts[:n_load]), N, K, WEIGHT)
    host_load_s = time.perf_counter() - t0
    host_query_us, host_update_us, host_step_us, worst_composed, worst_host, banks_agree = [], [], [], 0.0, 0.0, True
    for b, (w, q) in enumerate(work):
        a = comem.query_one_vs_many(q['src'], q['dst'], q['neg'])
        c = c_comem.one_vs_many(w['src'], w['dst'], w['neg'], with_term)
        worst_composed = max(worst_composed, tr.rel_err(cpu(a), cpu(c)))
        e = bank.query_one_vs_many(q['src'], q['dst'], q['neg'])
        banks_agree &= bool(torch.equal(e.long(), c_bank.one_vs_many(w['src'], w['dst'], w['neg'])))
        if b < args.host_batches:
            hs, hd, hn, ht = cpu(w['src']), cpu(w['dst']), cpu(w['neg']), cpu(w['ts'])
            t0 = time.perf_counter()
            h = np.stack([h_comem.scores(np.repeat(hs[p], M + 1), np.concatenate([hd[p : p + 1], hn[p]]), query_dtype) for p in range(bs)])
            t1 = time.perf_counter()
            he = np.stack([h_bank(np.repeat(hs[p], M + 1), np.concatenate([hd[p : p + 1], hn[p]])) for p in range(bs)])
            (he + h) / 2
            t2 = time.perf_counter()
            h_comem.update(hs, hd, ht)
            t3 = time.perf_counter()
            h_bank.update(hs, hd, ht)
            t4 = time.perf_counter()
            host_query_us.append((t1 - t0) * 1e6)
            host_update_us.append((t3 - t2) * 1e6)
            host_step_us.append((t4 - t0) * 1e6)
            worst_host = max(worst_host, tr.rel_err(cpu(a), h))
            banks_agree &= bool(np.array_equal(he, cpu(e.long())))
        for p in (bank, comem, c_bank, c_comem):
            p.update(w['src'], w['dst'], w['ts'])
    bank.check()
    comem.check()
    offered = [bank._offered - bs * len(work), comem._offered - bs * len(work)]  # a pass over the list offers its batches once more
    rehashes_before_timing = comem.rehashes + bank.rehashes

    (nc, cc), calls_seen = alternating_medians([n_calls, c_calls])
    (nm, cm), many_seen = alternating_medians([n_many, c_many])
    (nu, cu), update_seen = alternating_medians([n_update, c_update])
    (ns, cs), step_seen = alternating_medians([n_step, c_step])
    comem.check()
    hq, hu, hs_ = statistics.median(host_query_us), statistics.median(host_update_us), statistics.median(host_step_us)
    return {
        'bench': 'base3_example_shape', 'query_dtype': query_dtype, 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'loaded': n_load,
        'num_nodes': N, 'k': K, 'batches_timed': len(work), 'bs': bs, 'negatives': M, 'queries_per_batch': bs * (M + 1),
        'pair_table_capacity': comem.capacity, 'pairs': len(c_comem.keys),
        'rehashes_while_timing': comem.rehashes + bank.rehashes - rehashes_before_timing,
        'native_vs_composed_rel_err': worst_composed, 'native_vs_host_rel_err': worst_host, 'edgebank_three_ways_agree': banks_agree,
        'native_tcomem_query_200_calls_us': round(nc, 1), 'composed_tcomem_query_200_calls_us': round(cc, 1),
        'native_tcomem_query_one_vs_many_us': round(nm, 1), 'composed_tcomem_query_one_vs_many_us': round(cm, 1),
        'native_tcomem_update_us': round(nu, 1), 'composed_tcomem_update_us': round(cu, 1),
        'native_base3_step_us': round(ns, 1), 'composed_base3_step_us': round(cs, 1), 'native_step_speedup_vs_composed': round(cs / ns, 2),
        'native_is_the_faster_step': bool(ns < cs),
        'host_tcomem_query_200_calls_us': round(hq, 1), 'host_tcomem_update_us': round(hu, 1), 'host_base3_step_us': round(hs_, 1),
        'native_step_speedup_vs_host': round(hs_ / ns, 1), 'host_tcomem_load_s': round(host_load_s, 2),
        'windows_us': {'tcomem_query_200_calls': calls_seen, 'tcomem_query_one_vs_many': many_seen, 'tcomem_update': update_seen, 'base3_step': step_seen},
    }  # fmt: skip


for query_dtype in ('int64', 'float32'):
    print(json.dumps(run(query_dtype)), flush=True)
