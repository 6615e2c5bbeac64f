#!/usr/bin/env python
"""ROLAND at the shapes of examples/linkproppred/roland.py (wiki-shaped stream cut into hourly snapshots: 9 227 nodes, about 210 edges a
snapshot, node dim 256, embed dim 256).  What is timed, per snapshot, in microseconds, in eval mode, the embeddings of each snapshot fed
into the next:

  native     ROLAND.forward: one native call (tgmx_roland_forward)
  torch_ops  the same forward written HERE from stock torch ops on the device (index_add_ for the propagation, matmul, GRUCell /
             F.linear, clone of the embeddings passed in); this code calls none of the library's kernels

  learnable, gru, mlp   the hourly snapshots under each update ('learnable' is the example's default)
  heavy_*               ONE snapshot holding the whole stream (157 474 edges), the same three updates

A timed window loops over the snapshot list until it lasts at least --window-s seconds; the two variants take turns (one window each,
three rounds, after a warm-up window each) and each figure is the median of its three windows.  Also timed, GEMMs alone: the GRU update's
two plain GEMMs ([N, C] x [3C, C], twice) against one block-structured GEMM ([N, 2C] x [4C, 2C]).  Prints one JSON line; --out appends it.
    python tools/bench_roland.py [--snapshots S] [--out profiles/rNN_bench_roland.jsonl]"""
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
from tgm_amd.nn import ROLAND, _ops  # noqa: E402
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


class TorchOps:
    """ROLAND from stock torch ops (no edge weights, self loops added); dropped edges keep their slot with weight 0 (no read back)."""

    def __init__(self, model):
        self.m, self.update = model, model.update
        self.prev = [torch.zeros(N, EMBED, device=dev), torch.zeros(N, EMBED, device=dev)]

    def conv(self, conv, h, src, dst, w, dinv, diag):
        xw = torch.matmul(h, conv.lin.weight.t())
        return (diag.unsqueeze(1) * xw).index_add_(0, dst, (dinv[src] * w * dinv[dst]).unsqueeze(1) * xw[src]) + conv.bias

    def __call__(self, x, ei, prev=None):
        if prev is not None:
            self.prev = [prev[0].clone(), prev[1].clone()]
        src, dst = ei[0].long(), ei[1].long()
        w = (src != dst).float()
        deg = torch.ones(x.shape[0], device=dev).index_add_(0, dst, w)  # an explicit unweighted self loop weighs what the added one does
        dinv = deg.pow(-0.5)
        diag = dinv * dinv
        h, out = x, []
        for l, conv in enumerate((self.m.conv1, self.m.conv2)):
            h = F.relu(self.conv(conv, h, src, dst, w, dinv, diag))
            if self.update == 'gru':
                h = getattr(self.m, f'gru{l + 1}')(h, self.prev[l])
            elif self.update == 'mlp':
                h = getattr(self.m, f'mlp{l + 1}')(torch.cat((h, self.prev[l]), dim=1))
            else:
                h = self.m.tau * self.prev[l] + (1 - self.m.tau) * h
            out.append(h)
        return out


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


def shape(tag, update, snaps):
    torch.manual_seed(1)
    model = ROLAND(NODE_DIM, EMBED, N, dropout=0.1, update=update).to(dev).eval()
    if update == 'learnable':
        model.tau.fill_(0.3)
    ops = TorchOps(model)

    def run(step):
        prev = None
        for ei in snaps:
            prev = step(x, ei, prev)
        return prev

    native, torch_ops = (lambda: run(model)), (lambda: run(ops))
    (tn, tt), seen = alternating_medians([native, torch_ops], len(snaps))
    a, b = native(), torch_ops()
    model.check()
    agree = max(float(((p - q).abs() / q.abs().clamp(min=1)).max()) for p, q in zip(a, b))
    return {f'{tag}_snapshots': len(snaps), f'{tag}_edges_per_snapshot': round(statistics.mean(e.shape[1] for e in snaps), 1),
            f'{tag}_native_us_per_snapshot': round(tn, 1), f'{tag}_torch_ops_us_per_snapshot': round(tt, 1), f'{tag}_native_speedup': round(tt / tn, 2),
            f'{tag}_windows_us': seen, f'{tag}_native_vs_torch_ops_max_rel_diff': agree}  # fmt: skip


with torch.no_grad():
    line = {'bench': 'roland_example_shape', 'device': torch.cuda.get_device_name(0), 'num_nodes': N, 'node_dim': NODE_DIM, 'embed_dim': EMBED}
    for update in ('learnable', 'gru', 'mlp'):
        line.update(shape(update, update, hourly))
    for update in ('learnable', 'gru', 'mlp'):
        line.update(shape(f'heavy_{update}', update, [ei_all]))
    # the GRU update's GEMMs alone: two plain ones against one block-structured one (rows r, z: [W_ih | W_hh]; n: [W_ih_n | 0], [0 | W_hh_n])
    C = EMBED
    op, w_ih, w_hh, wb = torch.randn(N, 2 * C, device=dev), torch.randn(3 * C, C, device=dev), torch.randn(3 * C, C, device=dev), torch.randn(4 * C, 2 * C, device=dev)
    gi, gh, g4, b3, b4 = torch.empty(N, 3 * C, device=dev), torch.empty(N, 3 * C, device=dev), torch.empty(N, 4 * C, device=dev), torch.randn(3 * C, device=dev), torch.randn(4 * C, device=dev)

    def two_plain():
        _ops.sgemm_nt(op[:, :C], w_ih, gi, bias=b3)
        _ops.sgemm_nt(op[:, C:], w_hh, gh, bias=b3)

    (t2, t1), seen = alternating_medians([two_plain, lambda: _ops.sgemm_nt(op, wb, g4, bias=b4)], 1)
    line.update({'gru_gemm_two_plain_us': round(t2, 1), 'gru_gemm_one_block_us': round(t1, 1), 'gru_gemm_windows_us': seen})
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
