#!/usr/bin/env python
"""Generate the ROLAND fixtures tests/golden/g24_roland_*.npz by running the REFERENCE's ``ROLAND`` class (tgm/nn/encoder/roland.py).

Runs only where the reference checkout is.  PyG is not installed; the placeholder under tests/golden/_pyg_stub has a ``GCNConv`` restated
from the published definition and an empty ``Linear``, so this script sets ``torch_geometric.nn.Linear = torch.nn.Linear`` (same keys and
default initialisation) BEFORE the reference is imported.  What the fixtures pin is the reference's layer wiring, update rules, parameter
names and state handling around that convolution.  Every parameter is drawn here, uniform(-0.6, 0.6).

Recorded as plain .npz data:

    meta                  input_channel, out_channel, num_nodes, update, tau, snapshots, counts (per snapshot: num_current_edges,
                          num_previous_edges as passed, null where not passed)
    p.<state_dict key>    the parameters (float32)
    x{s}, ei{s}           snapshot s: node features [N, in] float32, edge_index [2, E] int64
    H0_{s}, H1_{s}        the reference's two embeddings after snapshot s (those of snapshot s - 1 fed back in; None at s = 0)

    python tests/golden/make_golden_roland.py

The float32 restatement (tests/roland_restate.py) must reproduce every recorded output within 1e-5 of max(1, |ref|) before anything is
written.

  g24_roland_learnable            tau a parameter, set to 0.3
  g24_roland_learnable_default    tau a parameter at its initial 0
  g24_roland_moving               tau from edge counts that differ per snapshot; the first call passes none (tau stays 0)
  g24_roland_fixed_tau            update=None, tau = 0.7
  g24_roland_gru, g24_roland_mlp  the GRUCell / Linear updates
  g24_roland_loops_dups_isolated  directed; several self loops on one node, repeated edges, nodes without in-edges
  g24_roland_empty_snapshot       a snapshot with E = 0 between two others
  g24_roland_odd_widths           input_channel 7, out_channel 5
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_pyg_stub'))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch_geometric.nn  # noqa: E402  (the placeholder)

import roland_restate as rr  # noqa: E402

torch_geometric.nn.Linear = torch.nn.Linear
import tgm.nn.encoder.roland as ref_roland  # noqa: E402

assert ref_roland.Linear is torch.nn.Linear and ref_roland.GCNConv is torch_geometric.nn.GCNConv


def fixture(name, N, cin, C, update, snaps, tau=0.5, set_tau=None, counts=None, seed=0) -> None:
    """snaps: per snapshot edge_index [2, E] int64; counts: per snapshot (num_current_edges, num_previous_edges) or (None, None)"""
    g = torch.Generator().manual_seed(seed)
    model = ref_roland.ROLAND(cin, C, N, dropout=0.0, update=update, tau=tau).eval()
    with torch.no_grad():
        for key, p in model.named_parameters():
            if key != 'tau':
                p.copy_(torch.empty(p.shape).uniform_(-0.6, 0.6, generator=g))
        if set_tau is not None:
            model.tau.fill_(set_tau)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == rr.expected_shapes(cin, C, update), name
    counts = counts or [(None, None)] * len(snaps)
    arrays = {f'p.{k}': v.numpy() for k, v in sd.items()}
    prev = None
    for s, ei in enumerate(snaps):
        x = torch.randn(N, cin, generator=g)
        ei = torch.as_tensor(ei, dtype=torch.int64).reshape(2, -1)
        out = model(x, ei, prev, *counts[s])
        assert all(not h.requires_grad and h.dtype == torch.float32 and h.shape == (N, C) for h in out)
        prev = out
        arrays[f'x{s}'], arrays[f'ei{s}'] = x.numpy(), ei.numpy()
        arrays[f'H0_{s}'], arrays[f'H1_{s}'] = out[0].numpy().copy(), out[1].numpy().copy()
    meta = dict(input_channel=cin, out_channel=C, num_nodes=N, update=update, tau=float(sd['tau']) if update == 'learnable' else tau,
                snapshots=len(snaps), counts=[list(c) for c in counts])  # fmt: skip
    loaded = [dict(x=torch.from_numpy(arrays[f'x{s}']), edge_index=torch.from_numpy(arrays[f'ei{s}']), counts=tuple(counts[s])) for s in range(len(snaps))]
    for s, (h0, h1) in rr.restated_replay(meta, sd, loaded, dtype=torch.float32):
        rr.close(h0, arrays[f'H0_{s}'], f'{name} H0 {s}')
        rr.close(h1, arrays[f'H1_{s}'], f'{name} H1 {s}')
    path = os.path.join(HERE, f'g24_roland_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    size = os.path.getsize(path)
    assert size < 40_000, (name, size)
    print(f'g24_roland_{name}: {size} bytes, {len(snaps)} snapshots, E = {[int(np.asarray(e).reshape(2, -1).shape[1]) for e in snaps]}')


def rand_edges(rng, N, E, lo_src=0, hi_src=None, lo_dst=0, hi_dst=None):
    return np.stack([rng.integers(lo_src, hi_src or N, E), rng.integers(lo_dst, hi_dst or N, E)]).astype(np.int64)


def both_ways(ei):
    return np.concatenate([ei, ei[::-1]], axis=1)


def main() -> None:
    rng = np.random.default_rng(2400)
    fixture('learnable', 24, 6, 8, 'learnable', [both_ways(rand_edges(rng, 24, n)) for n in (20, 31, 12, 26)], set_tau=0.3, seed=1)
    fixture('learnable_default', 20, 4, 8, 'learnable', [both_ways(rand_edges(rng, 20, n)) for n in (15, 22, 9)], seed=2)
    snaps = [both_ways(rand_edges(rng, 22, n)) for n in (14, 30, 9, 21)]
    sizes = [ei.shape[1] for ei in snaps]
    counts = [(None, None)] + [(sizes[s], sizes[s - 1]) for s in range(1, 4)]
    assert len({c[1] / (c[0] + c[1]) for c in counts[1:]}) == 3
    fixture('moving', 22, 5, 8, 'moving', snaps, counts=counts, seed=3)
    fixture('fixed_tau', 18, 4, 6, None, [both_ways(rand_edges(rng, 18, n)) for n in (16, 11, 19)], tau=0.7, seed=4)
    fixture('gru', 20, 6, 8, 'gru', [both_ways(rand_edges(rng, 20, n)) for n in (18, 25, 13, 20)], seed=5)
    fixture('mlp', 20, 6, 8, 'mlp', [both_ways(rand_edges(rng, 20, n)) for n in (18, 25, 13)], seed=6)
    snaps = []
    for n in (30, 44, 25):
        ei = rand_edges(rng, 30, n, 0, 12, 6, 18)  # sources 0..11, destinations 6..17: nodes 0..5 and 18..29 have no in-edges
        ei = ei[:, ei[0] != ei[1]]
        loops = np.array([[7, 7, 7, 9, 20], [7, 7, 7, 9, 20]])  # three loops on node 7, one on a node with in-edges, one on an isolated node
        ei = np.concatenate([ei, loops, ei[:, :6]], axis=1)  # six edges twice
        ei = ei[:, rng.permutation(ei.shape[1])]
        assert (ei[0] == ei[1]).sum() == 5 and len(set(map(tuple, ei.T))) < ei.shape[1] - 2
        snaps.append(ei)
    fixture('loops_dups_isolated', 30, 5, 8, 'learnable', snaps, set_tau=0.4, seed=7)
    fixture('empty_snapshot', 12, 4, 6, 'gru', [both_ways(rand_edges(rng, 12, 14)), np.zeros((2, 0), np.int64), both_ways(rand_edges(rng, 12, 10))], seed=8)
    fixture('odd_widths', 16, 7, 5, 'mlp', [both_ways(rand_edges(rng, 16, n)) for n in (16, 11, 19)], seed=9)


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
