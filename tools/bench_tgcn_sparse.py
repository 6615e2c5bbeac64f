#!/usr/bin/env python
"""TGCN / GCNConv over the sparse adjacency against the dense route and against stock torch ops, at the shapes of
examples/linkproppred/{tgcn,gcn}.py: the wiki-shaped stream cut into hourly snapshots (9 227 nodes, about 210 edges a snapshot, the
snapshotting of tools/bench_gclstm.py), node dim 256, embed dim 128.  Every figure is microseconds per snapshot through Python -- a CALL
RATE with a device synchronise at the window's ends, not kernel time (no launch is traced here).

  tgcn_infer   TGCN.forward under no_grad: propagate='sparse', 'dense', and the cell composed HERE from composed_gcn_conv + nn.Linear
  tgcn_train   forward, a linear loss on the output, backward, SGD step, H detached between snapshots (the example's loop): the same
               three; the peak of torch.cuda.max_memory_allocated for sparse and dense
  encoder      a two-layer GCN encoder (conv, batch norm, relu, conv: the gcn.py example's stack), forward + backward: one GCNGraph
               shared by both layers, a CSR built per layer (propagate='sparse'), dense
  all_edges    ONE snapshot of all 157 474 edges, TGCN inference and training: sparse and composed
  sweep        N in {255, 1 024, 2 048, 4 096, 9 227, 16 384} at 210 edges a snapshot and at E = 8 N, TGCN inference and training, sparse and
               dense: where the two cross
  transpose    tgmx_csr_transpose alone and the propagate over its result alone (384 channels), at a wiki snapshot and at all edges

The variants of one line take turns: a warm-up window each (which also sizes the windows), then one timed window each, three rounds; a figure
is the median of its three windows and `spread` is (max - min) / median of them.  One JSON line per measurement; --out appends them.
    python tools/bench_tgcn_sparse.py [--window-s 0.3] [--out profiles/rNN_bench_tgcn_sparse.jsonl]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd.nn import TGCN, GCNConv, gcn_graph  # noqa: E402
from tgm_amd.nn._snapshot import csr_transpose, gcn_propagate, propagate_scratch  # noqa: E402
from tgm_amd.nn.tgcn import composed_gcn_conv  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--snapshots', type=int, default=16, help='hourly snapshots a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.3, help='least duration of a timed window')
ap.add_argument('--out', type=str, default=None, help='append the JSON lines to this file')
ap.add_argument('--only', type=str, default='', help='comma-separated subset of: tgcn,encoder,all_edges,sweep,transpose')
args = ap.parse_args()
only = set(filter(None, args.only.split(',')))

dev = torch.device('cuda', 0)
NODE_DIM, EMBED = 256, 128
s = make_stream('wiki')
hour = (s.ts // 3600).tolist()
cuts = [0] + [i for i in range(1, len(hour)) if hour[i] != hour[i - 1]] + [len(hour)]
ei_all = torch.stack([s.src, s.dst]).to(dev)  # int32, as the loader hands batches over
hourly = [ei_all[:, a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])][: args.snapshots]


def emit(line):
    line = {'device': torch.cuda.get_device_name(0), 'unit': 'us per snapshot, call rate through Python', **line}
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(json.dumps(line) + '\n')


def window(fn, count, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * count) * 1e6


def measure(fns, count):
    """{name: (median, spread, windows)}: warm each up, then one window each in turn, three rounds."""
    failed = {}
    for k, fn in list(fns.items()):
        try:
            window(fn, count)
        except (RuntimeError, NotImplementedError) as e:  # a variant torch cannot run (reported, not timed)
            failed[k] = {'error': f'{type(e).__name__}: {str(e)[:120]}'}
    fns = {k: fn for k, fn in fns.items() if k not in failed}
    reps ={k: max(1, math.ceil(args.window_s * 1e6 / (window(fn, count) * count))) for k, fn in fns.items()}
    seen = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            seen[k].append(window(fn, count, reps[k]))
    out = dict(failed)
    for k, v in seen.items():
        med = statistics.median(v)
        out[k] = {'us': round(med, 1), 'spread': round((max(v) - min(v)) / med, 3), 'windows_us': [round(x, 1) for x in v]}
    return out


def composed_cell(cell, x, ei, H):
    """The cell from stock torch ops: composed_gcn_conv (sort + segment sums) per gate and nn.Linear."""
    H = torch.zeros(x.shape[0], cell.out_channels, device=x.device) if H is None else H
    cu, cr, cc = (composed_gcn_conv(c, x, ei) for c in (cell.conv_u, cell.conv_r, cell.conv_c))
    U = torch.sigmoid(cell.linear_u(torch.cat([cu, H], dim=1)))
    R = torch.sigmoid(cell.linear_r(torch.cat([cr, H], dim=1)))
    Ht = torch.tanh(cell.linear_c(torch.cat([cc, H * R], dim=1)))
    return U * H + (1 - U) * Ht


def tgcn_runners(N, snaps, in_dim, routes):
    """{('infer' | 'train', route): fn} over one cell per route with the same weights."""
    torch.manual_seed(0)
    x, wout = torch.randn(N, in_dim, device=dev), torch.randn(N, EMBED, device=dev)
    base = TGCN(in_dim, EMBED).to(dev)
    infer, train = {}, {}
    for r in routes:
        cell = TGCN(in_dim, EMBED, propagate='sparse' if r == 'composed' else r).to(dev)
        cell.load_state_dict(base.state_dict())
        opt = torch.optim.SGD(cell.parameters(), lr=1e-4)
        step = (lambda c: (lambda x, ei, H: composed_cell(c, x, ei, H)))(cell) if r == 'composed' else (lambda c: (lambda x, ei, H: c(x, ei, None, H)))(cell)

        def run_infer(step=step):
            with torch.no_grad():
                H = None
                for ei in snaps:
                    H = step(x, ei, H)
            return H

        def run_train(step=step, opt=opt):
            H = None
            for ei in snaps:
                opt.zero_grad(set_to_none=True)
                H = step(x, ei, H)
                (H * wout).sum().backward()
                opt.step()
                H = H.detach()
            return H

        infer[r], train[r] = run_infer, run_train
    return infer, train


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def agree(a, b):
    return float(((a - b).abs() / b.abs().clamp(min=1)).max())


def bench_tgcn(tag, N, snaps, routes, memory=False, extra=None):
    infer, train = tgcn_runners(N, snaps, NODE_DIM, routes)
    outs = {r: fn() for r, fn in infer.items()}  # same seeded inputs: the routes must agree before their times are compared
    line = {'bench': tag, 'num_nodes': N, 'snapshots': len(snaps), 'edges_per_snapshot': round(statistics.mean(e.shape[1] for e in snaps), 1),
            'node_dim': NODE_DIM, 'embed_dim': EMBED, **(extra or {})}  # fmt: skip
    line['infer_max_rel_diff_vs_sparse'] = {r: agree(o, outs['sparse']) for r, o in outs.items() if r != 'sparse'}
    line['infer'] = measure(infer, len(snaps))
    line['train'] = measure(train, len(snaps))
    if memory:
        line['train_peak_bytes_over_baseline'] = {r: peak_memory(train[r]) for r in routes if r != 'composed'}
    emit(line)


class Encoder(nn.Module):
    """Two GCN layers with batch norm and relu in between (the stack of the gcn.py examples at num_layers = 2, dropout off)."""

    def __init__(self, route):
        super().__init__()
        self.c1, self.bn, self.c2 = GCNConv(NODE_DIM, EMBED, propagate=route), nn.BatchNorm1d(EMBED), GCNConv(EMBED, EMBED, propagate=route)

    def forward(self, x, e):
        return self.c2(torch.relu(self.bn(self.c1(x, e))), e)


def bench_encoder():
    N = s.num_nodes
    torch.manual_seed(0)
    x, wout = torch.randn(N, NODE_DIM, device=dev), torch.randn(N, EMBED, device=dev)
    base = Encoder('auto').to(dev)
    fns = {}
    for name, route in (('shared_graph', 'auto'), ('csr_per_layer', 'sparse'), ('dense', 'dense')):
        enc = Encoder(route).to(dev)
        enc.load_state_dict(base.state_dict())

        def run(enc=enc, shared=name == 'shared_graph'):
            for ei in hourly:
                e = gcn_graph(ei, num_nodes=N) if shared else ei
                enc.zero_grad(set_to_none=True)
                (enc(x, e) * wout).sum().backward()

        fns[name] = run
    emit({'bench': 'gcn_encoder_fwd_bwd', 'num_nodes': N, 'snapshots': len(hourly), 'layers': 2, 'node_dim': NODE_DIM, 'embed_dim': EMBED,
          'fwd_bwd': measure(fns, len(hourly))})  # fmt: skip


def synthetic(N, E, count, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, N, (2, E), generator=g).to(torch.int32).to(dev) for _ in range(count)]


def bench_transpose(tag, ei):
    N, C = s.num_nodes, 3 * EMBED
    graph = gcn_graph(ei, num_nodes=N)
    csr_t = graph.transposed()
    t_in, t_out = torch.randn(N, C, device=dev), torch.empty(N, C, device=dev)
    scratch = propagate_scratch(csr_t, C)
    rows = (csr_t[0][1:] - csr_t[0][:-1])
    res = measure({'csr_transpose': lambda: csr_transpose(graph.csr, N),
                   'transposed_propagate': lambda: gcn_propagate(csr_t, t_in, t_out, scratch=scratch, E=graph.E)}, 1)  # fmt: skip
    emit({'bench': f'transpose_{tag}', 'num_nodes': N, 'edges': int(ei.shape[1]), 'entries': int(csr_t[0][-1]), 'longest_transposed_row': int(rows.max()),
          'channels': C, 'note': 'csr_transpose includes the allocation of its outputs and workspace', **res})  # fmt: skip


want = lambda k: not only or k in only
if want('tgcn'):
    bench_tgcn('tgcn_wiki_hourly', s.num_nodes, hourly, ('sparse', 'dense', 'composed'), memory=True)
if want('encoder'):
    bench_encoder()
if want('all_edges'):
    bench_tgcn('tgcn_all_edges_one_snapshot', s.num_nodes, [ei_all], ('sparse', 'composed'))
if want('sweep'):
    for N in (255, 1024, 2048, 4096, 9227, 16384):
        for E, label in ((210, '210_edges'), (8 * N, '8N_edges')):
            bench_tgcn('tgcn_sweep', N, synthetic(N, E, 4, N + E), ('sparse', 'dense'), extra={'edges': label})
if want('transpose'):
    bench_transpose('wiki_snapshot', hourly[0])
    bench_transpose('all_edges', ei_all)
