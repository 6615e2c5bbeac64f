#!/usr/bin/env python
"""The decoders at the shapes of the examples (examples/linkproppred/tgat.py and its siblings: batch size 200, about 1 000 candidates per
positive edge in evaluation; examples/nodeproppred, examples/graphproppred).  Per call, in microseconds, in eval mode without gradients:

  native     tgm_amd.nn.{LinkPredictor, NodePredictor, GraphPredictor}
  torch_ops  the reference's modules written HERE from stock torch ops on the device (cat / Linear / ReLU / mean); this code calls none of
             the library's kernels

  train_D        the training step's decoder work: decoder(z_src, z_dst) twice (positives, negatives) at R = 200, D = H in {100, 172}
  eval_D         the evaluation step: the examples' loop -- per positive edge index z twice and run the decoder on 1 + 999 rows, 200 times --
                 against ONE query_one_vs_many; z holds the unique nodes of a wiki-shaped batch and its negatives
  eval_D_table / eval_D_pair   the same call with the form pinned
  forms          score_pairs at R = 50 000 pairs, D = H = 172, over tables of N' = R / 16 .. 4 R rows, each form pinned: where they cross
  node           NodePredictor at R = 200, in = 172, out = 10
  graph          GraphPredictor (mean pooling) at N = 9 227, in = H = 128

A timed window repeats the call until it lasts at least --window-s seconds; the two variants take turns (one window each, three rounds,
after a warm-up window each) and each figure is the median of its three windows.  Prints one JSON line; --out appends it.
    python tools/bench_decoders.py [--out profiles/rNN_bench_decoders.jsonl]"""
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
from tgm_amd.nn import GraphPredictor, LinkPredictor, NodePredictor  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--window-s', type=float, default=0.3, help='least duration of a timed window')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()
dev = torch.device('cuda', 0)
BS, M = 200, 999


class TorchLink(nn.Module):
    """LinkPredictor with ConcatMerge from stock torch ops, sharing the native module's parameters."""

    def __init__(self, native):
        super().__init__()
        self.model = native.model

    def forward(self, z_src, z_dst):
        return self.model(torch.cat([z_src, z_dst], dim=1)).view(-1)


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def alternating_medians(fns):
    """Warm each up (which also sizes its window), then one window each in turn, three rounds: drift of the device hits all alike."""
    for fn in fns:
        window(fn)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / window(fn))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(v, 1) for v in vs] for vs in seen]


def entry(tag, names, fns, check=None):
    med, seen = alternating_medians(fns)
    out = {f'{tag}_{n}_us': round(t, 1) for n, t in zip(names, med)}
    out[f'{tag}_windows_us'] = seen
    if 'torch_ops' in names and 'native' in names:
        out[f'{tag}_native_speedup'] = round(med[names.index('torch_ops')] / med[names.index('native')], 2)
    if check is not None:
        out[f'{tag}_max_rel_diff'] = check()
    return out


def rel(a, b):
    return float(((a - b).abs() / b.abs().clamp(min=1)).max())


def pinned(form, fn):
    def run():
        os.environ['TGMX_DECODER_FORM'] = form
        try:
            return fn()
        finally:
            del os.environ['TGMX_DECODER_FORM']

    return run


with torch.no_grad():
    line = {'bench': 'decoders_example_shape', 'device': torch.cuda.get_device_name(0), 'batch_size': BS, 'candidates': M}
    # a wiki-shaped evaluation batch: the unique nodes of 200 edges and of 999 negative destinations each
    s = make_stream('wiki')
    lo = s.src.numel() // 2
    src_ids, dst_ids = s.src[lo : lo + BS].long(), s.dst[lo : lo + BS].long()
    g = torch.Generator().manual_seed(0)
    d_lo, d_hi = int(s.dst.min()), int(s.dst.max()) + 1
    neg_ids = torch.randint(d_lo, d_hi, (BS, M), generator=g)
    uniq = torch.unique(torch.cat([src_ids, dst_ids, neg_ids.reshape(-1)]))
    src_idx, dst_idx, neg_idx = (torch.searchsorted(uniq, t).to(dev) for t in (src_ids, dst_ids, neg_ids))
    NP = uniq.numel()
    line.update({'eval_table_rows': NP, 'eval_pairs': BS * (M + 1)})
    for D in (100, 172):
        torch.manual_seed(D)
        dec = LinkPredictor(D, hidden_dim=D).to(dev).eval()
        ref = TorchLink(dec)
        z = torch.randn(NP, D, device=dev)
        a, b, c = z[:BS].contiguous(), z[BS : 2 * BS].contiguous(), z[2 * BS : 3 * BS].contiguous()
        line.update(entry(f'train_{D}', ['native', 'torch_ops'], [lambda: (dec(a, b), dec(a, c)), lambda: (ref(a, b), ref(a, c))],
                          lambda: rel(dec(a, b), ref(a, b))))  # fmt: skip

        def loop(model):
            out = []
            for i in range(BS):
                d_i = torch.cat([dst_idx[i : i + 1], neg_idx[i]])
                s_i = src_idx[i].repeat(M + 1)
                out.append(model(z[s_i], z[d_i]))
            return out

        many = lambda: dec.query_one_vs_many(z, src_idx, dst_idx, neg_idx)
        line.update(entry(f'eval_{D}', ['native', 'torch_ops', 'native_loop'], [many, lambda: loop(ref), lambda: loop(dec)],
                          lambda: rel(many().reshape(-1), torch.cat(loop(ref)))))  # fmt: skip
        line.update(entry(f'eval_{D}_forms', ['table', 'pair'], [pinned('table', many), pinned('pair', many)]))
    # where the two forms cross
    D, R = 172, 50_000
    torch.manual_seed(1)
    dec = LinkPredictor(D, hidden_dim=D).to(dev).eval()
    for ratio in (1 / 16, 1 / 4, 1 / 2, 1, 2, 4):
        n = int(R * ratio)
        z = torch.randn(n, D, device=dev)
        ia, ib = torch.randint(0, n, (R,), device=dev, dtype=torch.int32), torch.randint(0, n, (R,), device=dev, dtype=torch.int32)
        line.update(entry(f'forms_ratio_{ratio:g}', ['table', 'pair'], [pinned('table', lambda: dec.score_pairs(z, ia, ib)), pinned('pair', lambda: dec.score_pairs(z, ia, ib))]))
    del z
    torch.manual_seed(2)
    node = NodePredictor(172, 10, hidden_dim=172).to(dev).eval()
    x = torch.randn(BS, 172, device=dev)
    line.update(entry('node', ['native', 'torch_ops'], [lambda: node(x), lambda: node.model(x)], lambda: rel(node(x), node.model(x))))
    graph = GraphPredictor(128, hidden_dim=128).to(dev).eval()
    zn = torch.randn(9227, 128, device=dev)
    stock = lambda: graph.model(torch.mean(zn, dim=0).squeeze())
    line.update(entry('graph', ['native', 'torch_ops'], [lambda: graph(zn), stock], lambda: rel(graph(zn), stock())))
    dec.check()
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
