"""GraphAttentionEmbedding's share of a TGN training step -- forward, a linear loss, backward -- on a wiki-shaped batch (bs = 200, k = [10]:
600 unique nodes at most, 6000 sampled edges at most, 172 message columns).

  dims = 100 (memory = time = embed = 100, C = 50): the one-node path (TGMX_TGN_BWD=native) against the default path, alternating in one process
  dims = 172 (C = 86): the one-node path against the same layer composed from stock torch ops (index_add softmax), alternating

Method: warm-up, then per side the median of WINDOWS windows of at least 0.5 s, each ending in a synchronise; two runs of the whole
comparison.  One JSON line per (dims, run) is appended to profiles/r36_bench_tgn_train.jsonl (or --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINDOWS, WINDOW_S = 3, 0.5


def stock_layer(enc, x, lu, edge_index, t, msg):
    """The layer from stock torch ops (dropout off): what a user would write without the library."""
    conv, src, tgt = enc.conv, edge_index[0], edge_index[1]
    H, C = conv.heads, conv.out_channels
    rel = (lu[src] - t).float().unsqueeze(-1)
    attr = torch.cat([torch.cos(enc.time_enc.w(rel)), msg], -1)
    e = conv.lin_edge(attr).view(-1, H, C)
    q, k, v = (lin(x).view(-1, H, C) for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
    s = (q[tgt] * (k[src] + e)).sum(-1) / C ** 0.5
    m = torch.full((x.shape[0], H), -float('inf'), device=x.device).scatter_reduce(0, tgt[:, None].expand(-1, H), s, 'amax')
    w = torch.exp(s - m[tgt])
    a = w / torch.zeros(x.shape[0], H, device=x.device).index_add_(0, tgt, w)[tgt]
    out = torch.zeros(x.shape[0], H, C, device=x.device).index_add_(0, tgt, a[..., None] * (v[src] + e))
    return conv.lin_skip(x) + out.view(-1, H * C)


def measure(step):
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                step()
            n += 10
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S:
                break
        per.append(dt / n * 1e6)
    return per


def main():
    from tgm_amd.nn import GraphAttentionEmbedding, Time2Vec

    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r36_bench_tgn_train.jsonl'))
    ap.add_argument('--runs', type=int, default=2)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    U, E, D = 600, 6000, 172
    edge_index = torch.from_numpy(rng.integers(0, U, (2, E)).astype(np.int64)).to(dev)
    lu = torch.from_numpy(rng.integers(0, 2_000_000, U).astype(np.int64)).to(dev)
    t = torch.from_numpy(rng.integers(0, 2_000_000, E).astype(np.int64)).to(dev)
    msg = torch.from_numpy(rng.random((E, D), dtype=np.float32)).to(dev)
    for dims in (100, 172):
        torch.manual_seed(0)
        enc = GraphAttentionEmbedding(dims, dims, D, Time2Vec(dims)).to(dev).train()
        enc.conv.dropout = 0.1 if dims == 100 else 0.0  # (the stock composition has no counter-based mask: both sides without dropout at 172)
        x = torch.randn(U, dims, device=dev, requires_grad=True)
        G = torch.randn(U, dims, device=dev)

        def step(fn=None):
            for p in enc.parameters():
                p.grad = None
            x.grad = None
            z = enc(x, lu, edge_index, t, msg) if fn is None else fn(enc, x, lu, edge_index, t, msg)
            (z * G).sum().backward()

        def native_step():
            os.environ['TGMX_TGN_BWD'] = 'native'
            step()

        def default_step():
            os.environ.pop('TGMX_TGN_BWD', None)
            step()

        other, other_name = (default_step, 'default_path') if dims == 100 else (lambda: step(stock_layer), 'stock_torch')
        for run in range(args.runs):
            a, b = [], []
            for _ in range(2):  # alternate the two sides inside a run
                a += measure(native_step)
                b += measure(other)
            rec = dict(tool='bench_tgn_train', dims=dims, C=dims // 2, U=U, E=E, run=run, device=torch.cuda.get_device_name(0),
                       one_node_us=statistics.median(a), one_node_windows_us=[round(v, 1) for v in a],
                       **{f'{other_name}_us': statistics.median(b), f'{other_name}_windows_us': [round(v, 1) for v in b]},
                       ratio=statistics.median(b) / statistics.median(a))
            print(json.dumps(rec), flush=True)
            with open(args.out, 'a') as f:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
