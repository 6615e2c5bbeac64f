#!/usr/bin/env python
"""TGBNegativeEdgeSamplerHook per evaluation batch, in microseconds, at two shapes:

  wiki   23 621 positives x 999 negatives each (ids below 9 227), bs = 200: the validation split of tgbl-wiki in shape
  wide   100 000 positives x 100 negatives each (ids below 1 000 000), bs = 4096

measured three ways in the same process, on the same device-resident batches:

  native      tgm_amd.hooks.TGBNegativeEdgeSamplerHook.from_eval_set (csrc/tgbneg.hip): the table built once (timed once, upload included),
              then per batch the probe / copy / mark launch, the bitmap compaction and one read of the statistics
  delegating  the same hook over a sampler object whose evaluation set is no dict: ``query_batch`` on the host, one padded matrix up, the
              same compaction
  composed    the reference's algorithm, written here: the batch to the host, a dictionary lookup and a list of Python integers per
              positive, ``torch.tensor(list)`` per positive on the device, ``cat``, ``unique``, ``min().item()``, ``max().item()``, ``randint``

and the EdgeBank evaluation step (hook + ``query_one_vs_many`` + ``update``) with ``batch.neg_batch_list`` handed over as it is (its matrix is
taken) against the same entries as a plain list (``B`` tensors are concatenated).

A timed window is K consecutive batches between two device synchronisations, on a host clock; the variants' windows alternate; each figure
is the median of --windows windows, the spread (min .. max) is reported beside it.  Before timing, the three variants' answers for one batch
are compared.  Appends one JSON line per shape to --out (profiles/r29_bench_tgbneg.jsonl holds two runs).
    python tools/bench_tgbneg.py [--out FILE] [--shapes wiki,wide]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgm_amd.hooks import TGBNegativeEdgeSamplerHook  # noqa: E402
from tgm_amd.nn import EdgeBankPredictor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29_bench_tgbneg.jsonl'))
ap.add_argument('--shapes', default='wiki,wide')
ap.add_argument('--windows', type=int, default=9)
ap.add_argument('--scale', type=float, default=1.0, help='shrink the number of positives (checks of the script)')
ap.add_argument('--rehearse-on-cpu', action='store_true', help='run the script on host tensors: checks the script, times nothing of interest, writes no file')
args = ap.parse_args()

if args.rehearse_on_cpu:
    dev, sync = torch.device('cpu'), (lambda: None)
else:
    assert torch.cuda.is_available(), 'bench_tgbneg.py measures on a ROCm device'
    dev, sync = torch.device('cuda', 0), torch.cuda.synchronize

SHAPES = {'wiki': dict(P=23_621, Q=999, N=9_227, bs=200, K=20), 'wide': dict(P=100_000, Q=100, N=1_000_000, bs=4096, K=8)}


class LookupSampler:
    """a sampler object as the hook's delegating path sees it: query_batch is a lookup, the evaluation set is not a dict the hook may flatten"""

    def __init__(self, ev, split):
        self._ev, self.eval_set = ev, {split: None}

    def query_batch(self, src, dst, ts, split_mode='val'):
        ev = self._ev
        return [ev[k] for k in zip(src.tolist(), dst.tolist(), ts.tolist())]


def composed(ev, batch):
    """the reference's __call__ with TGB's query_batch in front of it"""
    rows = [ev[k].tolist() for k in zip(batch.edge_src.tolist(), batch.edge_dst.tolist(), batch.edge_time.tolist())]
    neg_list = [torch.tensor(r, dtype=torch.int32, device=dev) for r in rows]
    neg = torch.unique(torch.cat(neg_list))
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    neg_time = torch.randint(int(batch.edge_time.min().item()), int(batch.edge_time.max().item()) + 1, (neg.size(0),), device=dev, generator=gen)
    return neg, neg_list, neg_time


def spread(v):
    return [round(min(v), 1), round(max(v), 1)]


def run(shape: str) -> dict:
    cfg = SHAPES[shape]
    P, Q, N, bs, K = max(2 * cfg['bs'], int(cfg['P'] * args.scale)), cfg['Q'], cfg['N'], cfg['bs'], cfg['K']
    rng = np.random.default_rng(29)
    src, dst = rng.integers(0, N, P), rng.integers(0, N, P)
    ts = np.sort(rng.integers(1_000_000, 3_000_000, P))
    t0 = time.perf_counter()
    negs = rng.integers(0, N, (P, Q)).astype(np.int32)
    ev = {(int(s), int(d), int(t)): negs[p] for p, (s, d, t) in enumerate(zip(src, dst, ts))}
    P = len(ev)
    keys = np.array(list(ev), dtype=np.int64)
    host_set_s = time.perf_counter() - t0
    dg = types.SimpleNamespace(device=dev)
    nb = (P + bs - 1) // bs
    batches = []
    for b in range(nb):
        k = keys[b * bs : (b + 1) * bs]
        T = lambda col, dt: torch.from_numpy(np.ascontiguousarray(k[:, col])).to(dt).to(dev)
        batches.append((T(0, torch.int32), T(1, torch.int32), T(2, torch.int64)))
    fresh = lambda b: types.SimpleNamespace(edge_src=batches[b % nb][0], edge_dst=batches[b % nb][1], edge_time=batches[b % nb][2])

    sync()
    t0 = time.perf_counter()
    native = TGBNegativeEdgeSamplerHook.from_eval_set(ev)
    first = native(dg, fresh(0))
    sync()
    build_s = time.perf_counter() - t0  # flatten on the host, upload, the insert launch, its status read, and the first batch
    deleg = TGBNegativeEdgeSamplerHook.from_eval_set({(0, 0, 0): np.zeros(1, dtype=np.int64)})
    deleg.neg_sampler, deleg._eval, deleg._flat, deleg._delegating = LookupSampler(ev, 'val'), None, None, True
    deleg._query_batch = lambda batch: deleg.neg_sampler.query_batch(batch.edge_src, batch.edge_dst, batch.edge_time, split_mode='val')

    # the three answers agree before anything is timed
    c_neg, c_list, c_time = composed(ev, fresh(0))
    second = deleg(dg, fresh(0))
    for got in (first, second):
        assert got.neg.dtype == c_neg.dtype and torch.equal(got.neg, c_neg) and torch.equal(got.neg_time, c_time)
        assert all(torch.equal(x, y) for x, y in zip(got.neg_batch_list, c_list)) and len(got.neg_batch_list) == len(c_list)

    steps = {'native': lambda b: native(dg, fresh(b)), 'delegating': lambda b: deleg(dg, fresh(b)), 'composed': lambda b: composed(ev, fresh(b))}

    # the EdgeBank evaluation step
    hist = (torch.from_numpy(rng.integers(0, N, 50_000)).int().to(dev), torch.from_numpy(rng.integers(0, N, 50_000)).int().to(dev),
            torch.from_numpy(np.sort(rng.integers(0, 1_000_000, 50_000))).to(dev))  # fmt: skip
    if not args.rehearse_on_cpu:
        bank = EdgeBankPredictor(*hist)

        def eval_step(b, plain):
            batch = native(dg, fresh(b))
            negs_ = list(batch.neg_batch_list) if plain else batch.neg_batch_list
            out = bank.query_one_vs_many(batch.edge_src, batch.edge_dst, negs_)
            bank.update(batch.edge_src, batch.edge_dst, batch.edge_time)
            return out

        a, c = bank.query_one_vs_many(first.edge_src, first.edge_dst, first.neg_batch_list), bank.query_one_vs_many(first.edge_src, first.edge_dst, list(first.neg_batch_list))
        assert len(a) == len(c) and all(torch.equal(x, y) for x, y in zip(a, c))  # before any update moves the memory
        steps['edgebank_step_matrix'] = lambda b: eval_step(b, False)
        steps['edgebank_step_list'] = lambda b: eval_step(b, True)

    def window(step, first_batch):
        sync()
        t0 = time.perf_counter()
        for b in range(first_batch, first_batch + K):
            step(b)
        sync()
        return (time.perf_counter() - t0) / K * 1e6

    for step in steps.values():  # warm every variant
        window(step, 0)
    times = {name: [] for name in steps}
    for w in range(args.windows):
        for name, step in steps.items():
            times[name].append(window(step, w * K))
    out = dict(bench='tgb_negatives', shape=shape, device=torch.cuda.get_device_name(0) if dev.type == 'cuda' else 'cpu', positives=P, negatives_each=Q,
               num_ids=N, bs=bs, batches_per_window=K, windows=args.windows, host_set_s=round(host_set_s, 2), native_build_and_first_batch_s=round(build_s, 3),
               table_capacity=native._state(dev).capacity if dev.type == 'cuda' else 0, qpad=first.neg_batch_list.matrix.shape[1],
               unique_first_batch=int(first.neg.numel()))  # fmt: skip
    for name, v in times.items():
        out[name + '_us'] = round(statistics.median(v), 1)
        out[name + '_us_spread'] = spread(v)
    out['native_speedup_over_composed'] = round(out['composed_us'] / out['native_us'], 1)
    out['native_speedup_over_delegating'] = round(out['delegating_us'] / out['native_us'], 1)
    return out


for name in args.shapes.split(','):
    line = json.dumps(run(name))
    print(line, flush=True)
    if not args.rehearse_on_cpu:
        with open(args.out, 'a') as f:
            f.write(line + '\n')
