#!/usr/bin/env python
"""GCLSTM training steps at the shapes of examples/linkproppred/gclstm.py (wiki-shaped stream cut into hourly snapshots: 9 227 nodes, about
210 edges a snapshot, node dim 256, embed dim 256), K = 1 (the example's) and K = 3.  What is timed, per step, in microseconds:

  native  the native training path: tgmx_gclstm_forward with the activations kept per call, tgmx_gclstm_backward as one call
  torch   TGMX_GCLSTM_BWD=torch: GCLSTM.forward_composed and autograd -- the training path as it was before the native one, unchanged

  (a) example  one snapshot a step, as the example runs it: h_0 / c_0 detached, node features without gradient; cell forward, a linear
               loss on relu(H), backward, an SGD step (so the stacked weights are rebuilt every step, as in real training)
  (b) bptt     two snapshots a step, the states carried with their graph from the first into the second; the same loss after the second

A timed window loops over the snapshot list until it lasts at least --window-s seconds and ends in a synchronise; the two paths take
turns in one process (one window each, three rounds, after a warm-up window each) and each figure is the median of its three windows.
Prints one JSON line; --out appends it.
    python tools/bench_gclstm_train.py [--snapshots S] [--out profiles/rNN_bench_gclstm_train.jsonl]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd.nn import GCLSTM  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--snapshots', type=int, default=48, help='hourly snapshots a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()

dev = torch.device('cuda', 0)
NODE_DIM = EMBED = 256
s = make_stream('wiki')
N = s.num_nodes
hour = (s.ts // 3600).tolist()
cuts = [0] + [i for i in range(1, len(hour)) if hour[i] != hour[i - 1]] + [len(hour)]
ei_all = torch.stack([s.src, s.dst]).to(dev)  # int32, as the loader hands batches over
hourly = [ei_all[:, a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])][: args.snapshots]
torch.manual_seed(0)
x = torch.randn(N, NODE_DIM, device=dev)
w_loss = torch.randn(N, EMBED, device=dev) / N


def window(fn, count, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * count) * 1e6


def alternating_medians(fns, count):
    """Warm each up (which also sizes its window), then one window each in turn, three rounds: drift of the device hits all alike."""
    for fn in fns:
        window(fn, count)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / (window(fn, count) * count))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, count, reps[i]))
    return [statistics.median(v) for v in seen], [[round(v, 1) for v in vs] for vs in seen]


def make_runner(K, path, per_step):
    """(a function that runs one pass over the snapshot list, the cell): ``per_step`` snapshots between two backward calls."""
    torch.manual_seed(1)
    cell = GCLSTM(NODE_DIM, EMBED, K).to(dev).train()
    opt = torch.optim.SGD(cell.parameters(), lr=1e-6)
    want = 'Gclstm' if path == 'native' else 'Mul'

    def run():
        if path == 'torch':
            os.environ['TGMX_GCLSTM_BWD'] = 'torch'
        else:
            os.environ.pop('TGMX_GCLSTM_BWD', None)
        h = c = None
        for i in range(0, len(hourly) - per_step + 1, per_step):
            opt.zero_grad(set_to_none=True)
            for ei in hourly[i : i + per_step]:
                h, c = cell(x, ei, None, h, c)
            assert want in type(h.grad_fn).__name__, type(h.grad_fn).__name__
            (torch.relu(h) * w_loss).sum().backward()
            opt.step()
            h, c = h.detach(), c.detach()
        os.environ.pop('TGMX_GCLSTM_BWD', None)
        return h, c

    return run, cell


def shape(tag, K, per_step):
    (native, cell_n), (composed, cell_t) = make_runner(K, 'native', per_step), make_runner(K, 'torch', per_step)
    steps = len(hourly) // per_step
    (tn, tt), seen = alternating_medians([native, composed], steps)
    (Hn, _), (Ht, _) = native(), composed()
    cell_n.check()
    cell_t.check()
    agree = float(((Hn - Ht).abs() / Ht.abs().clamp(min=1)).max())  # (the same number of SGD steps from the same start on both)
    return {f'{tag}_K': K, f'{tag}_snapshots_per_step': per_step, f'{tag}_steps_per_window_pass': steps,
            f'{tag}_edges_per_snapshot': round(statistics.mean(e.shape[1] for e in hourly), 1), f'{tag}_native_us_per_step': round(tn, 1),
            f'{tag}_torch_us_per_step': round(tt, 1), f'{tag}_native_speedup': round(tt / tn, 2), f'{tag}_windows_us': seen,
            f'{tag}_native_vs_torch_max_rel_diff_H': agree}  # fmt: skip


line = {'bench': 'gclstm_train_example_shape', 'device': torch.cuda.get_device_name(0), 'num_nodes': N, 'node_dim': NODE_DIM, 'embed_dim': EMBED}
line.update(shape('example_k1', 1, 1))
line.update(shape('example_k3', 3, 1))
line.update(shape('bptt_k1', 1, 2))
line.update(shape('bptt_k3', 3, 2))
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
