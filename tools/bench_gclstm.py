#!/usr/bin/env python
"""GCLSTM at the shapes of examples/linkproppred/gclstm.py (wiki-shaped stream cut into hourly snapshots: 9 227 nodes, about 210 edges a
snapshot, node dim 256, embed dim 256).  What is timed, per snapshot, in microseconds, under no_grad:

  native     GCLSTM.forward: one native call (tgmx_gclstm_forward)
  torch_ops  the same forward written HERE from stock torch ops on the device (index_add_ for the propagation, matmul, pointwise ops);
             this code calls none of the library's kernels

  (a) example  K = 1 (the example's setting: the graph is not read)
  (b) k3       the same snapshots, K = 3
  (c) heavy    ONE snapshot holding the whole stream (157 474 edges), K = 3; the propagate launch (tgmx_cheb_propagate, 256 channels) is
               also timed on its own and its gathered bytes per second (entries x 1 KiB / time) set against the 8 TB/s HBM specification

A timed window loops over the snapshot list until it lasts at least --window-s seconds; the two variants take turns (one window each,
three rounds, after a warm-up window each) and each figure is the median of its three windows.  Prints one JSON line; --out appends it.
    python tools/bench_gclstm.py [--snapshots S] [--out profiles/rNN_bench_gclstm.jsonl]"""
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
from tgm_amd.nn import gclstm as product  # noqa: E402
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


def torch_ops_forward(p, K, x, ei, H, C):
    """The cell from stock torch ops ('sym', lambda_max 2, no edge weights); dropped edges keep their slot with weight 0 (no read back)."""
    n = x.shape[0]
    H = torch.zeros(n, EMBED, device=dev) if H is None else H
    C = torch.zeros(n, EMBED, device=dev) if C is None else C
    tx = [H]
    if K > 1:
        row, col = ei[0].long(), ei[1].long()
        w = (row != col).float()
        deg = torch.zeros(n, device=dev).index_add_(0, row, w)
        dis = deg.pow(-0.5)
        dis = dis.masked_fill(dis == float('inf'), 0)
        m = -(dis[row] * w * dis[col])  # times 2 / lambda_max = 1; the diagonal 2 / lambda_max - 1 = 0
        apply = lambda t: torch.zeros_like(t).index_add_(0, col, m.unsqueeze(1) * t[row])
        tx.append(apply(H))
        for _ in range(2, K):
            tx.append(2.0 * apply(tx[-1]) - tx[-2])
    pre = []
    for g in 'ifco':
        v = torch.matmul(x, p[f'W_{g}'])
        for k in range(K):
            v = v + torch.matmul(tx[k], p[f'conv_{g}.lins.{k}.weight'].t())
        pre.append(v + p[f'conv_{g}.bias'] + p[f'b_{g}'])
    I, F, T, O = torch.sigmoid(pre[0]), torch.sigmoid(pre[1]), torch.tanh(pre[2]), torch.sigmoid(pre[3])
    C = F * C + I * T
    return O * torch.tanh(C), C


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


def shape(tag, K, snaps):
    torch.manual_seed(1)
    cell = GCLSTM(NODE_DIM, EMBED, K).to(dev).eval()
    p = {k: v.detach() for k, v in cell.state_dict().items()}

    def native():
        H = C = None
        for ei in snaps:
            H, C = cell(x, ei, None, H, C)
        return H, C

    def torch_ops():
        H = C = None
        for ei in snaps:
            H, C = torch_ops_forward(p, K, x, ei, H, C)
        return H, C

    (tn, tt), seen = alternating_medians([native, torch_ops], len(snaps))
    (Hn, Cn), (Ht, Ct) = native(), torch_ops()
    cell.check()
    agree = max(float(((a - b).abs() / b.abs().clamp(min=1)).max()) for a, b in ((Hn, Ht), (Cn, Ct)))
    width = NODE_DIM + K * EMBED
    return {f'{tag}_K': K, f'{tag}_snapshots': len(snaps), f'{tag}_edges_per_snapshot': round(statistics.mean(e.shape[1] for e in snaps), 1),
            f'{tag}_native_us_per_snapshot': round(tn, 1), f'{tag}_torch_ops_us_per_snapshot': round(tt, 1), f'{tag}_native_speedup': round(tt / tn, 2),
            f'{tag}_gemm_gflop': round(2 * N * 4 * EMBED * width / 1e9, 2), f'{tag}_windows_us': seen, f'{tag}_native_vs_torch_ops_max_rel_diff': agree}  # fmt: skip


with torch.no_grad():
    line = {'bench': 'gclstm_example_shape', 'device': torch.cuda.get_device_name(0), 'num_nodes': N, 'node_dim': NODE_DIM, 'embed_dim': EMBED}
    line.update(shape('example', 1, hourly))
    line.update(shape('k3', 3, hourly))
    line.update(shape('heavy', 3, [ei_all]))
    # the propagate launch of the heavy snapshot on its own
    lap = product.scaled_laplacian(ei_all, None, N, 'sym', 2.0, None)
    t_in, t_out = torch.randn(N, EMBED, device=dev), torch.empty(N, EMBED, device=dev)
    entries = int(lap[0][-1].item())
    scratch = product.propagate_scratch(lap, EMBED)
    (tp,), seen = alternating_medians([lambda: product.propagate(lap, t_in, t_out, scratch=scratch)], 1)
    rows = lap[0][1:] - lap[0][:-1]
    line.update({'heavy_propagate_us': round(tp, 1), 'heavy_propagate_entries': entries, 'heavy_propagate_longest_row': int(rows.max()),
                 'heavy_propagate_gathered_TBps': round(entries * EMBED * 4 / (tp * 1e-6) / 1e12, 3),
                 'heavy_propagate_fraction_of_8TBps': round(entries * EMBED * 4 / (tp * 1e-6) / 8e12, 3), 'heavy_propagate_windows_us': seen})  # fmt: skip
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
