#!/usr/bin/env python
"""DensityOfStateEstimatorHook per batch, in microseconds, on two batch shapes and three snapshot shapes:

  wiki      the example's setting (examples/analytics/dos.py): the wiki-shaped stream, bs = 200, 20 moments, 100 probes, 1001 points
  comment   the comment-shaped stream (1 000 000 nodes), bs = 4096, its first --comment-edges events, the same estimator
  wiki_day  a snapshot: the first 5 200 events of the wiki-shaped stream (9 227 ids) as ONE batch (csrc/dos_large.hip past 4096 events)
  snap64k   a snapshot: 65 536 uniform events over 100 000 ids
  snap1m    a snapshot: the first 1 000 000 events of the comment-shaped stream (1 000 000 ids)

Measured in the same process:

  native     the hook on device tensors (csrc/dos.hip, one call of three launches), with sync=False (nothing read) and sync=True (one read)
  composed   the hook's ``_estimate_composed``: the same definition from stock torch ops on the device in float32 (``unique``,
             ``index_put``, a dense [n, n] operator, ``matmul``), its result left on the device
  host       wiki only: the hook's numpy float64 path on host copies of the batches (the copies are made outside the window)

A timed window is K consecutive batches between two device synchronisations, on a host clock; each figure is the median of --windows
windows with the spread beside it, and native and composed windows alternate so that a pair shares the machine's state.  Before anything is
reported the two ways are compared on one batch.  Where the composed path cannot allocate its dense operator the line says so instead of
giving a time.  Appends one JSON line per shape to --out (the snapshot shapes: profiles/r39_bench_dos_large.jsonl).
    python tools/bench_dos.py [--out FILE] [--shapes wiki,comment,wiki_day,snap64k,snap1m]"""
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
from tgm_amd.hooks import DensityOfStateEstimatorHook  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r38_bench_dos.jsonl'))
ap.add_argument('--shapes', default='wiki,comment')
ap.add_argument('--comment-edges', type=int, default=1_000_000)
ap.add_argument('--windows', type=int, default=9)
ap.add_argument('--step-seconds', type=float, default=40.0)
ap.add_argument('--rehearse-on-cpu', action='store_true', help='run the script on host tensors: checks the script, times nothing of interest, writes no file')
args = ap.parse_args()

if args.rehearse_on_cpu:
    dev, sync = torch.device('cpu'), lambda: None
else:
    assert torch.cuda.is_available(), 'bench_dos.py measures on a ROCm device'
    dev, sync = torch.device('cuda', 0), torch.cuda.synchronize
MOMENTS, PROBES, POINTS, SEED = 20, 100, 1001, 1337


def spread(v):
    return {'median': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1), 'windows': len(v)}


def stream(shape: str, edges: int):
    if shape == 'snap64k':
        gen = torch.Generator().manual_seed(SEED)
        return tuple(torch.randint(0, 100_000, (edges,), generator=gen, dtype=torch.int32).to(dev) for _ in range(2))
    s = make_stream({'wiki_day': 'wiki', 'snap1m': 'comment'}.get(shape, shape), num_edges=edges, edge_dim=0)
    return s.src.to(dev), s.dst.to(dev)


def run(shape: str, bs: int, edges: int, K: int) -> dict:
    src, dst = stream(shape, edges)
    per_pass = edges // bs

    def batch(i, to=None):
        lo = (i % per_pass) * bs
        b = types.SimpleNamespace(edge_src=src[lo : lo + bs], edge_dst=dst[lo : lo + bs])
        return b if to is None else types.SimpleNamespace(edge_src=b.edge_src.to(to), edge_dst=b.edge_dst.to(to))

    new = lambda **kw: DensityOfStateEstimatorHook(MOMENTS, PROBES, POINTS, seed=SEED, **kw)

    def composed_step():
        h = new(sync=False)
        h._rng_seed = SEED

        def step(b):
            h.calls += 1
            return h._estimate_composed(b.edge_src, b.edge_dst)

        return step

    steps = {
        'native_nosync': (lambda h: lambda b: h(None, b))(new(sync=False)),
        'native_sync': (lambda h: lambda b: h(None, b))(new()),
        'composed': composed_step(),
    }
    cannot = None
    for name, step in list(steps.items()):
        try:
            for i in range(5):
                step(batch(i))
        except torch.OutOfMemoryError as e:  # the composed path's dense [n, n] operator
            assert name == 'composed'
            cannot = 'cannot allocate: ' + str(e).split('.')[0]
            del steps[name]
            torch.cuda.empty_cache()
    # windows of the three ways interleaved: window w of each runs over the same K batches
    out = {k: [] for k in steps}
    t_end = time.perf_counter() + args.step_seconds
    for w in range(args.windows):
        if w and time.perf_counter() > t_end:
            break
        batches = [batch(i) for i in range(5 + w * K, 5 + (w + 1) * K)]
        for k, step in steps.items():
            sync()
            t0 = time.perf_counter()
            for b in batches:
                step(b)
            sync()
            out[k].append((time.perf_counter() - t0) / K * 1e6)
    result = {k: spread(v) for k, v in out.items()}
    if shape == 'wiki':
        host = new()
        hb = [batch(i, 'cpu') for i in range(K)]
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            for b in hb:
                host(None, b)
            times.append((time.perf_counter() - t0) / K * 1e6)
        result['host_numpy'] = spread(times)
    # the two ways on one batch (both as call 1 of the same seed): the float32 paths agree to the forward bar of each against float64
    b = batch(3)
    a, c = new(sync=False), new(sync=False)
    native = a(None, types.SimpleNamespace(**vars(b))).dos.cpu().numpy()
    head = {
        'bench': 'dos_hook', 'shape': shape, 'device': torch.cuda.get_device_name(0) if dev.type == 'cuda' else 'cpu (rehearsal)', 'bs': bs,
        'moments': MOMENTS, 'probes': PROBES, 'n_pts': POINTS, 'batches_per_window': K, 'native_path': a.last_path,
    }  # fmt: skip
    if cannot:
        return {**head, 'composed': cannot, 'per_kernel_us': 'not measured', 'us_per_batch': result}
    c._rng_seed, c.calls = SEED, 1
    composed = c._estimate_composed(b.edge_src, b.edge_dst).cpu().numpy()
    return {
        **head,
        'native_vs_composed_max_diff_of_max': float(np.abs(native - composed).max() / composed.max()),
        'native_faster_in_every_window_pair': bool(all(n < c for n, c in zip(out['native_sync'], out['composed'])) and all(n < c for n, c in zip(out['native_nosync'], out['composed']))),
        'speedup_nosync': round(result['composed']['median'] / result['native_nosync']['median'], 1),
        'speedup_sync': round(result['composed']['median'] / result['native_sync']['median'], 1),
        'per_kernel_us': 'not measured',
        'us_per_batch': result,
    }  # fmt: skip


SHAPES = {'wiki': (200, 157_474, 50), 'comment': (4096, args.comment_edges, 20),
          'wiki_day': (5200, 5200, 5), 'snap64k': (65536, 65536, 2), 'snap1m': (1_000_000, 1_000_000, 1)}  # fmt: skip
for name in args.shapes.split(','):
    bs, edges, K = SHAPES[name]
    line = json.dumps(run(name, bs, edges, K))
    print(line, flush=True)
    if not args.rehearse_on_cpu:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')
