#!/usr/bin/env python
"""HistoricalNegativeEdgeSamplerHook per batch, early in a stream and after at least a million events, in microseconds:

  wiki      the wiki-shaped stream (157 474 events over 8 227 sources), bs = 200; passes over it repeat until the position is reached
            (the hook keeps every event it is offered, so a repeated pass grows the histories like new events would)
  comment   the comment-shaped stream (1 000 000 nodes), bs = 4096, its first --comment-edges events

measured two ways in the same process:

  native     tgm_amd.hooks.HistoricalNegativeEdgeSamplerHook on device tensors (csrc/histneg.hip): one call per batch, nothing read back
  composed   the reference's algorithm from stock torch ops on the device, written here: ``isin`` of the whole log against the batch's
             sources, ``unique`` with inverse, a lookup table sized by ``max().item()``, one ``rand`` per matching event, a scatter-max,
             the two masked writes, then the batch written behind the log (capacity doubling)

A timed window is K consecutive batches between two device synchronisations, on a host clock.  "early": a new sampler, 20 batches to
warm it, then the window (so the window starts 20 batches into the stream, every time).  "late": the sampler is taken through the stream
batch by batch (native) or has the same events loaded into its log (composed) until --late-events are in, then the windows follow one
another down the stream.  Native and composed windows alternate; each figure is the median of --windows windows, the spread is reported
beside it.  Appends one JSON line per shape to --out (profiles/r17_bench_histneg.jsonl holds two runs).
    python tools/bench_histneg.py [--out FILE] [--shapes wiki,comment]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgm_amd import DGData, DGraph  # noqa: E402
from tgm_amd.hooks import HistoricalNegativeEdgeSamplerHook  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_bench_histneg.jsonl'))
ap.add_argument('--shapes', default='wiki,comment')
ap.add_argument('--late-events', type=int, default=1_000_000)
ap.add_argument('--comment-edges', type=int, default=2_700_000)
ap.add_argument('--windows', type=int, default=9)
ap.add_argument('--warm-batches', type=int, default=20)
ap.add_argument('--rehearse-on-cpu', action='store_true', help='run the script on host tensors at whatever size is given: checks the script, times nothing of interest, writes no file')
args = ap.parse_args()

if args.rehearse_on_cpu:
    dev = torch.device('cpu')
    sync = lambda: None
else:
    assert torch.cuda.is_available(), 'bench_histneg.py measures on a ROCm device'
    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize


class Composed:
    """the reference's sampler out of torch ops: the log is [2, cap] int32, `n` events in it"""

    def __init__(self):
        self.log, self.n = None, 0

    def load(self, src, dst):
        self.n = src.numel()
        self.log = torch.zeros((2, 2 * self.n), dtype=torch.int32, device=dev)
        self.log[0, : self.n], self.log[1, : self.n] = src, dst

    def __call__(self, src, dst, ts):
        B = src.numel()
        if self.n == 0:
            neg = torch.full((B,), -1, dtype=dst.dtype, device=dev)
        else:
            past_src, past_dst = self.log[0, : self.n], self.log[1, : self.n]
            hit = torch.isin(past_src, src)
            cand_src, cand_dst = past_src[hit], past_dst[hit]
            uniq, inverse = torch.unique(src, return_inverse=True)
            slot_of = torch.zeros(int(src.max().item()) + 1, dtype=torch.long, device=dev)
            slot_of[uniq.long()] = torch.arange(uniq.numel(), device=dev)
            cand_slot = slot_of[cand_src.long()]
            weight = torch.rand(cand_src.numel(), device=dev)
            best = torch.full((uniq.numel(),), -1.0, device=dev).scatter_reduce_(0, cand_slot, weight, reduce='amax')
            winner = weight == best[cand_slot]
            per_source = torch.full((uniq.numel(),), -1, dtype=torch.int32, device=dev)
            per_source[cand_slot[winner]] = cand_dst[winner]
            neg = per_source[inverse]
        out = neg, ts.clone(), neg != -1
        if self.log is None:
            self.log = torch.zeros((2, 2 * B), dtype=torch.int32, device=dev)
        if self.n + B > self.log.shape[1]:
            grown = torch.zeros((2, max(2 * self.log.shape[1], 2 * (self.n + B))), dtype=torch.int32, device=dev)
            grown[:, : self.log.shape[1]] = self.log
            self.log = grown
        self.log[0, self.n : self.n + B], self.log[1, self.n : self.n + B] = src, dst
        self.n += B
        return out


def spread(v):
    return {'median': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)}


def run(shape: str, bs: int, edges: int, K: int) -> dict:
    s = make_stream(shape, num_edges=edges, edge_dim=0)
    dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1)), device=dev)
    src, dst, ts = s.src.to(dev), s.dst.to(dev), s.ts.to(dev)
    per_pass = edges // bs

    def batch(b):  # batch b of the endless stream (pass after pass)
        lo = (b % per_pass) * bs
        return types.SimpleNamespace(edge_src=src[lo : lo + bs], edge_dst=dst[lo : lo + bs], edge_time=ts[lo : lo + bs])

    def timed(step, first):
        sync()
        t0 = time.perf_counter()
        for b in range(first, first + K):
            step(batch(b))
        sync()
        return (time.perf_counter() - t0) / K * 1e6

    W = args.warm_batches
    n_step = lambda hook: (lambda b: hook(dg, b))
    c_step = lambda comp: (lambda b: comp(b.edge_src, b.edge_dst, b.edge_time))

    def early(make, step_of):
        obj = make()
        for b in range(W):
            step_of(obj)(batch(b))
        return timed(step_of(obj), W)

    early(HistoricalNegativeEdgeSamplerHook, n_step), early(Composed, c_step)  # code objects, allocator, algorithm choices
    n_early, c_early = [], []
    for _ in range(args.windows):
        n_early.append(early(HistoricalNegativeEdgeSamplerHook, n_step))
        c_early.append(early(Composed, c_step))

    late_batches = -(-args.late_events // bs)
    hook = HistoricalNegativeEdgeSamplerHook(seed=17)
    t0 = time.perf_counter()
    for b in range(late_batches):
        hook(dg, batch(b))
    sync()
    advance_s = time.perf_counter() - t0
    comp = Composed()
    comp.load(hook._memory[0, : hook._count], hook._memory[1, : hook._count])
    hook.check()
    probe = batch(late_batches)  # same answer to "has this source a past event" from both, at the late position
    probe = types.SimpleNamespace(edge_src=probe.edge_src.clone(), edge_dst=probe.edge_dst.clone(), edge_time=probe.edge_time.clone())
    masks_agree = bool(torch.equal(hook(dg, probe).valid_neg_mask, comp(probe.edge_src, probe.edge_dst, probe.edge_time)[2]))
    timed(n_step(hook), late_batches + 1), timed(c_step(comp), late_batches + 1)
    n_late, c_late = [], []
    nxt = late_batches + 1 + K
    for _ in range(args.windows):
        n_late.append(timed(n_step(hook), nxt))
        c_late.append(timed(c_step(comp), nxt))
        nxt += K
    hook.check()
    ne, nl, ce, cl = (statistics.median(v) for v in (n_early, n_late, c_early, c_late))
    return {
        'bench': 'historical_negatives', 'shape': shape, 'device': torch.cuda.get_device_name(0) if dev.type == 'cuda' else 'cpu (rehearsal)',
        'bs': bs, 'stream_events': edges, 'num_nodes': s.num_nodes, 'batches_per_window': K, 'windows': args.windows,
        'early_window_starts_at_events': W * bs, 'late_window_starts_at_events': (late_batches + 1 + K) * bs, 'events_at_end': hook._count,
        'native_advance_to_late_s': round(advance_s, 2), 'pool_words': hook._dev['pool'].numel() if hook._dev else 0, 'pool_grown': hook.pool_grown,
        'masks_agree_at_late_position': masks_agree,
        'native_early_us': round(ne, 1), 'native_late_us': round(nl, 1), 'native_late_over_early': round(nl / ne, 2),
        'composed_early_us': round(ce, 1), 'composed_late_us': round(cl, 1), 'composed_late_over_early': round(cl / ce, 2),
        'native_speedup_early': round(ce / ne, 1), 'native_speedup_late': round(cl / nl, 1),
        'windows_us': {'native_early': spread(n_early), 'native_late': spread(n_late), 'composed_early': spread(c_early), 'composed_late': spread(c_late)},
    }  # fmt: skip


SHAPES = {'wiki': (200, 157_474, 100), 'comment': (4096, args.comment_edges, 30)}
for name in args.shapes.split(','):
    bs, edges, K = SHAPES[name]
    line = json.dumps(run(name, bs, edges, K))
    print(line, flush=True)
    if not args.rehearse_on_cpu:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')
