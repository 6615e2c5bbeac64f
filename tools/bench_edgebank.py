#!/usr/bin/env python
"""EdgeBankPredictor at the EdgeBank example's shape: a wiki-shaped stream, the table loaded with its first 70 %, then evaluation batches of
bs = 200 positives with 999 negatives each (200 000 queries a batch) followed by the batch's update.  Both memory modes.  Per batch, in
microseconds:

  query_200_calls        the example's loop: one call per positive edge (1 000 queries each), inputs built beforehand
  query_one_vs_many      the same answers from one ``query_one_vs_many`` call
  update                 ``update`` with the batch's 200 edges
  step                   query_one_vs_many + update, the evaluation step

each measured three ways in the same process:

  native     tgm_amd.nn.EdgeBankPredictor (csrc/edgebank.hip)
  composed   the same from torch ops on the device: the memory as sorted packed keys, a query is ``searchsorted``, the update is ``cat`` + a
             stable sort + keeping the last of every run of equal keys (boolean indexing: it synchronises, as ``unique`` does)
  host       the reference's algorithm on the host, a Python dict behind ``.tolist()`` (tests/edgebank_restate.py), on a few batches, once

A timed window loops over the batch list until it lasts at least --window-s seconds; the variants of one figure take turns (one window
each, three rounds, after a warm-up window each) and each figure is the median of its three windows.  The timed loops offer the same
batches again and again, which adds no pairs; the predictor's count of offered events is put back after every pass over the batch list,
so that the table keeps the size the stream gives it (the host sizes the table by events offered, it cannot see that they repeat).
Prints one JSON line per memory mode.
    python tools/bench_edgebank.py [--edges E] [--batches B]"""
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
from tgm_amd.nn import EdgeBankPredictor  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=157_474)
ap.add_argument('--batches', type=int, default=20, help='distinct batches a timed window loops over')
ap.add_argument('--host-batches', type=int, default=2, help='batches the host restatement is timed on')
ap.add_argument('--window-s', type=float, default=0.3, help='least duration of a timed window')
ap.add_argument('--negatives', type=int, default=999)
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, M = 200, args.negatives
s = make_stream('wiki', num_edges=args.edges, edge_dim=0)
n_load = int(0.7 * args.edges)
src, dst, ts = s.src.to(dev), s.dst.to(dev), s.ts.to(dev)
n_src = int(s.src.max()) + 1
gen = torch.Generator().manual_seed(11)
work = []
for b in range(args.batches):
    lo = n_load + b * bs
    neg = torch.randint(n_src, s.num_nodes, (bs, M), generator=gen, dtype=torch.int32).to(dev)  # destinations of the bipartite stream
    bsrc, bdst = src[lo : lo + bs], dst[lo : lo + bs]
    work.append(dict(src=bsrc, dst=bdst, ts=ts[lo : lo + bs], neg=neg, calls=[(bsrc[p].repeat(M + 1), torch.cat([bdst[p : p + 1], neg[p]])) for p in range(bs)]))


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


class Composed:
    """EdgeBank from torch ops on the device: sorted packed keys and their timestamps"""

    def __init__(self, src, dst, ts, fixed, ratio):
        self.fixed = fixed
        self.end = ts.max()
        start = ts.max() - ratio * (ts.max() - ts.min()) if fixed else ts.min()
        self.size = self.end - start
        self.keys = torch.empty(0, dtype=torch.int64, device=dev)
        self.ts = torch.empty(0, dtype=torch.int64, device=dev)
        self.update(src, dst, ts)

    def update(self, src, dst, ts):
        self.end = torch.max(self.end, ts.max())
        start = self.end - self.size
        ok = (ts.float() if self.fixed else ts) >= start
        keys = torch.cat([self.keys, (src.long() << 32 | dst.long())[ok]])
        tss = torch.cat([self.ts, ts[ok]])
        keys, order = torch.sort(keys, stable=True)  # equal keys stay in arrival order: the last of a run is the last arrival
        last = torch.ones_like(keys, dtype=torch.bool)
        last[:-1] = keys[1:] != keys[:-1]
        self.keys, self.ts = keys[last], tss[order][last]

    def query(self, src, dst):
        q = src.long() << 32 | dst.long()
        i = torch.searchsorted(self.keys, q).clamp_(max=self.keys.numel() - 1)
        hit = self.keys[i] == q
        if self.fixed:
            hit &= self.ts[i].double() >= (self.end - self.size).double()
        return hit.to(src.dtype)

    def one_vs_many(self, src, dst, neg):
        return self.query(src[:, None].expand(-1, neg.shape[1] + 1), torch.cat([dst[:, None], neg], 1))


def run(mode: str) -> dict:
    fixed = mode == 'fixed'
    native = EdgeBankPredictor(src[:n_load], dst[:n_load], ts[:n_load], memory_mode=mode)
    comp = Composed(src[:n_load], dst[:n_load], ts[:n_load], fixed, 0.15)
    offered = 0

    def keep_size():  # (see the module docstring)
        native._offered = offered

    def n_calls():
        for w in work:
            for qs, qd in w['calls']:
                native(qs, qd)

    def n_many():
        for w in work:
            native.query_one_vs_many(w['src'], w['dst'], w['neg'])

    def n_update():
        for w in work:
            native.update(w['src'], w['dst'], w['ts'])
        keep_size()

    def n_step():
        for w in work:
            native.query_one_vs_many(w['src'], w['dst'], w['neg'])
            native.update(w['src'], w['dst'], w['ts'])
        keep_size()

    def c_calls():
        for w in work:
            for qs, qd in w['calls']:
                comp.query(qs, qd)

    def c_many():
        for w in work:
            comp.one_vs_many(w['src'], w['dst'], w['neg'])

    def c_update():
        for w in work:
            comp.update(w['src'], w['dst'], w['ts'])

    def c_step():
        for w in work:
            comp.one_vs_many(w['src'], w['dst'], w['neg'])
            comp.update(w['src'], w['dst'], w['ts'])

    # agreement first, on the state the stream gives: every batch queried, then offered, three ways for the first host batches
    cpu = lambda t: t.cpu().numpy()
    host = er.EdgeBankRestated(cpu(src[:n_load]), cpu(dst[:n_load]), cpu(ts[:n_load]), mode, 0.15)
    host_query_us, host_update_us, agree = [], [], True
    for b, w in enumerate(work):
        a, c = native.query_one_vs_many(w['src'], w['dst'], w['neg']), comp.one_vs_many(w['src'], w['dst'], w['neg'])
        agree &= bool(torch.equal(a, c))
        if b < args.host_batches:
            hs, hd, hn = cpu(w['src']), cpu(w['dst']), cpu(w['neg'])
            t0 = time.perf_counter()
            h = np.stack([host(np.repeat(hs[p], M + 1), np.concatenate([hd[p : p + 1], hn[p]])) for p in range(bs)])
            host_query_us.append((time.perf_counter() - t0) * 1e6)
            agree &= bool(np.array_equal(h, cpu(a)))
            t0 = time.perf_counter()
            host.update(hs, hd, cpu(w['ts']))
            host_update_us.append((time.perf_counter() - t0) * 1e6)
        native.update(w['src'], w['dst'], w['ts'])
        comp.update(w['src'], w['dst'], w['ts'])
    native.check()
    offered = native._offered - bs * len(work)  # a pass over the list offers its batches once more
    rehashes_before_timing = native.rehashes
    hits = float(native.query_one_vs_many(work[-1]['src'], work[-1]['dst'], work[-1]['neg']).float().mean())

    (nc, cc), calls_seen = alternating_medians([n_calls, c_calls])
    (nm, cm), many_seen = alternating_medians([n_many, c_many])
    (nu, cu), update_seen = alternating_medians([n_update, c_update])
    (ns, cs), step_seen = alternating_medians([n_step, c_step])
    hq, hu = statistics.median(host_query_us), statistics.median(host_update_us)
    return {
        'bench': 'edgebank_example_shape', 'memory_mode': mode, 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'loaded': n_load,
        'batches_timed': len(work), 'bs': bs, 'negatives': M, 'queries_per_batch': bs * (M + 1), 'capacity': native.capacity,
        'entries': len(comp.keys), 'rehashes': native.rehashes, 'rehashes_while_timing': native.rehashes - rehashes_before_timing, 'hit_rate_last_batch': round(hits, 4), 'three_ways_agree': agree,
        'native_query_200_calls_us': round(nc, 1), 'composed_query_200_calls_us': round(cc, 1),
        'native_query_one_vs_many_us': round(nm, 1), 'composed_query_one_vs_many_us': round(cm, 1),
        'native_update_us': round(nu, 1), 'composed_update_us': round(cu, 1),
        'native_step_us': round(ns, 1), 'composed_step_us': round(cs, 1), 'native_step_speedup_vs_composed': round(cs / ns, 2),
        'native_is_the_faster_step': bool(ns < cs),
        'host_query_200_calls_us': round(hq, 1), 'host_update_us': round(hu, 1), 'native_step_speedup_vs_host': round((hq + hu) / ns, 1),
        'windows_us': {'query_200_calls': calls_seen, 'query_one_vs_many': many_seen, 'update': update_seen, 'step': step_seen},
    }  # fmt: skip


for mode in ('unlimited', 'fixed'):
    print(json.dumps(run(mode)), flush=True)
