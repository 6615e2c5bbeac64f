#!/usr/bin/env python
"""The decoder's share of a link-prediction training step at the shapes of the examples (examples/linkproppred/tgat.py's train(): batch
size 200, D = H in {100, 172}): the forward of the positive and the negative call, BCE with logits, and the backward down to ``z.grad``
and the parameters' gradients.  Per step, in microseconds:

  two_calls    native: decoder(z_src, z_dst), decoder(z_src, z_neg) -- the saving forward twice, tgmx_decoder_backward twice
  score_pairs  native: ONE decoder.score_pairs(z, ia, ib) over z [3 B, D] and the 2 B pairs (the table form: N' <= 2 R)
  torch        TGMX_DECODER_BWD=torch: the composed torch path, what the heads did before they had a backward

Every step ends with an optimizer step (SGD; all three variants pay it) so that whatever a variant caches against the parameters'
versions is rebuilt once per step, inside the timing.  A timed window repeats the step until it lasts at
least --window-s seconds; the variants take turns (one window each, three rounds, after a warm-up window each) and each figure is the
median of its three windows; the whole schedule runs twice (``runs``).  Prints one JSON line; --out appends it.
    python tools/bench_decoder_train.py [--out profiles/rNN_bench_decoder_train.jsonl]"""
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
from tgm_amd.nn import LinkPredictor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--window-s', type=float, default=0.15, help='least duration of a timed window')
ap.add_argument('--out', type=str, default=None, help='append the JSON line to this file')
args = ap.parse_args()
dev = torch.device('cuda', 0)
B = 200


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def alternating_medians(fns):
    for fn in fns:
        window(fn, 3)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / window(fn, 5))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(v, 1) for v in vs] for vs in seen]


def with_env(value, fn):
    def run():
        if value is None:
            os.environ.pop('TGMX_DECODER_BWD', None)
        else:
            os.environ['TGMX_DECODER_BWD'] = value
        try:
            return fn()
        finally:
            os.environ.pop('TGMX_DECODER_BWD', None)

    return run


line = {'bench': 'decoder_train_example_shape', 'device': torch.cuda.get_device_name(0), 'batch_size': B, 'runs': []}
for run in range(2):
    res = {}
    for D in (100, 172):
        torch.manual_seed(D)
        dec = LinkPredictor(D, hidden_dim=D).to(dev).train()
        opt = torch.optim.SGD(dec.parameters(), lr=1e-3)
        z0 = torch.randn(3 * B, D, device=dev)
        ar = torch.arange(B, device=dev)
        ia, ib = torch.cat((ar, ar)), torch.cat((ar + B, ar + 2 * B))
        ones, zeros = torch.ones(B, device=dev), torch.zeros(B, device=dev)
        target = torch.cat((ones, zeros))
        grads = {}

        def two_calls(tag='two_calls'):
            z = z0.detach().requires_grad_()
            opt.zero_grad(set_to_none=True)
            z_src, z_dst, z_neg = z[:B], z[B : 2 * B], z[2 * B :]
            loss = F.binary_cross_entropy_with_logits(dec(z_src, z_dst), ones) + F.binary_cross_entropy_with_logits(dec(z_src, z_neg), zeros)
            loss.backward()
            grads[tag] = [z.grad] + [p.grad for p in dec.parameters()]
            opt.step()

        def one_call():
            z = z0.detach().requires_grad_()
            opt.zero_grad(set_to_none=True)
            (2 * F.binary_cross_entropy_with_logits(dec.score_pairs(z, ia, ib), target)).backward()
            grads['score_pairs'] = [z.grad] + [p.grad for p in dec.parameters()]
            opt.step()

        fns = [with_env(None, two_calls), with_env(None, one_call), with_env('torch', lambda: two_calls('torch'))]
        # the three variants' gradients on the same, freshly drawn parameters (lr = 0: these steps change nothing).  Later in training a
        # hidden unit that sits at zero within rounding can take the other side of the ReLU in another variant: a whole term, not an error
        for group in opt.param_groups:
            group['lr'] = 0.0
        for fn in fns:
            fn()
        rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1)).max())
        res[f'train_{D}_max_rel_diff'] = max(max(rel(a, t), rel(b, t)) for a, b, t in zip(grads['two_calls'], grads['score_pairs'], grads['torch']))
        for group in opt.param_groups:
            group['lr'] = 1e-3
        med, seen = alternating_medians(fns)
        names = ['two_calls', 'score_pairs', 'torch']
        res.update({f'train_{D}_{n}_us': round(t, 1) for n, t in zip(names, med)})
        res[f'train_{D}_windows_us'] = seen
        res[f'train_{D}_two_calls_speedup'] = round(med[2] / med[0], 2)
        res[f'train_{D}_score_pairs_speedup'] = round(med[2] / med[1], 2)
        dec.check()
    line['runs'].append(res)
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
