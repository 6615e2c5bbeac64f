#!/usr/bin/env python
"""Generate the GCLSTM fixtures tests/golden/g23_gclstm_*.npz by running the REFERENCE's ``GCLSTM`` class (tgm/nn/encoder/gclstm.py).

Runs only where the reference checkout is.  PyG is not installed and the placeholder under tests/golden/_pyg_stub has an empty
``ChebConv``; this script installs a ``ChebConv`` restated from the published definition (tests/gclstm_restate.py, run in the input's dtype)
as ``torch_geometric.nn.ChebConv`` BEFORE the reference is imported, so what the fixtures pin is the reference's gate wiring, parameter
names and state handling around that convolution.  The placeholder's ``glorot`` does nothing: every parameter is drawn here.

Recorded as plain .npz data:

    meta                  in_channels, out_channels, K, normalization, bias, lambda_max, num_nodes, snapshots
    p.<state_dict key>    the parameters (float32)
    x{s}, ei{s}, ew{s}    snapshot s: node features [N, in] float32, edge_index [2, E] int64, edge weights [E] float32 (absent: unweighted)
    H{s}, C{s}            the reference's hidden and cell state after snapshot s (H, C of snapshot s - 1 fed back in; None at s = 0)

    python tests/golden/make_golden_gclstm.py

The float32 restatement must reproduce every recorded H, C within 1e-5 of max(1, |ref|) before anything is written.

  g23_gclstm_k1              K = 1: the examples' setting, where the graph is not read at all
  g23_gclstm_k2_weighted     K = 2 with edge weights
  g23_gclstm_k3_directed     one-directional edges; nodes that are only sources or only destinations; isolated nodes
  g23_gclstm_k4_loops_dups   self loops and repeated edges (weighted on the odd snapshots)
  g23_gclstm_rw_lmax         'rw' with lambda_max 2.5
  g23_gclstm_none_lmax       no normalisation with lambda_max 6.0
  g23_gclstm_empty_snapshot  a snapshot with E = 0 between two others
  g23_gclstm_nobias          bias=False
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

import gclstm_restate as gr  # noqa: E402


class ChebConv(torch.nn.Module):
    """``torch_geometric.nn.ChebConv`` restated: the parameters of the published layout, the arithmetic of tests/gclstm_restate.py."""

    def __init__(self, in_channels, out_channels, K, normalization='sym', bias=True, **kw):
        super().__init__()
        assert K > 0 and normalization in (None, 'sym', 'rw')
        self.normalization = normalization
        self.lins = torch.nn.ModuleList([torch.nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)

    def forward(self, x, edge_index, edge_weight=None, batch=None, lambda_max=None):
        return gr.cheb_conv([lin.weight for lin in self.lins], self.bias, x, edge_index, edge_weight, self.normalization, lambda_max, dtype=x.dtype)


torch_geometric.nn.ChebConv = ChebConv
import tgm.nn.encoder.gclstm as ref_gclstm  # noqa: E402

assert ref_gclstm.ChebConv is ChebConv


def fixture(name, N, cin, C, K, snaps, normalization='sym', bias=True, lambda_max=None, seed=0) -> None:
    """snaps: per snapshot (edge_index [2, E] int64, edge_weight or None)"""
    g = torch.Generator().manual_seed(seed)
    cell = ref_gclstm.GCLSTM(cin, C, K, normalization=normalization, bias=bias)
    with torch.no_grad():
        for p in cell.parameters():
            p.copy_(torch.empty(p.shape).uniform_(-0.6, 0.6, generator=g))
    sd = {k: v.detach().clone() for k, v in cell.state_dict().items()}
    assert sorted(sd) == sorted(gr.expected_shapes(cin, C, K, bias)) and {k: tuple(v.shape) for k, v in sd.items()} == gr.expected_shapes(cin, C, K, bias)
    arrays = {f'p.{k}': v.numpy() for k, v in sd.items()}
    lm = None if lambda_max is None else torch.tensor(lambda_max)
    H = C_ = H32 = C32 = None
    for s, (ei, ew) in enumerate(snaps):
        x = torch.randn(N, cin, generator=g)
        ei = torch.as_tensor(ei, dtype=torch.int64).reshape(2, -1)
        ew = None if ew is None else torch.as_tensor(ew, dtype=torch.float32)
        with torch.no_grad():
            H, C_ = cell(x, ei, ew, H, C_, lambda_max=lm)
        H32, C32 = gr.gclstm_forward(sd, x, ei, ew, H32, C32, lambda_max, normalization, dtype=torch.float32)
        assert H.dtype == torch.float32 and H.shape == (N, C)
        gr.close(H32, H, f'{name} H{s}')
        gr.close(C32, C_, f'{name} C{s}')
        arrays[f'x{s}'], arrays[f'ei{s}'], arrays[f'H{s}'], arrays[f'C{s}'] = x.numpy(), ei.numpy(), H.numpy().copy(), C_.numpy().copy()
        if ew is not None:
            arrays[f'ew{s}'] = ew.numpy()
    meta = dict(in_channels=cin, out_channels=C, K=K, normalization=normalization, bias=bias, lambda_max=lambda_max, num_nodes=N, snapshots=len(snaps))
    path = os.path.join(HERE, f'g23_gclstm_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    size = os.path.getsize(path)
    assert size < 40_000, (name, size)
    print(f'g23_gclstm_{name}: {size} bytes, {len(snaps)} snapshots, E = {[int(np.asarray(e).reshape(2, -1).shape[1]) for e, _ in snaps]}')


def rand_edges(rng, N, E, lo_src=0, hi_src=None, lo_dst=0, hi_dst=None):
    return np.stack([rng.integers(lo_src, hi_src or N, E), rng.integers(lo_dst, hi_dst or N, E)]).astype(np.int64)


def both_ways(ei):
    return np.concatenate([ei, ei[::-1]], axis=1)


def main() -> None:
    rng = np.random.default_rng(2300)
    w = lambda ei: rng.uniform(0.5, 2.0, ei.shape[1]).astype(np.float32)
    fixture('k1', 20, 5, 8, 1, [(both_ways(rand_edges(rng, 20, n)), None) for n in (15, 22, 9)], seed=1)
    snaps = [both_ways(rand_edges(rng, 24, n)) for n in (20, 31, 12, 26)]
    fixture('k2_weighted', 24, 4, 6, 2, [(ei, w(ei)) for ei in snaps], seed=2)
    # sources only 0..7, both 8..17, destinations only 18..23, isolated 24..29
    snaps = [rand_edges(rng, 30, n, 0, 18, 8, 24) for n in (60, 80, 50)]
    snaps = [ei[:, ei[0] < ei[1]] for ei in snaps]  # low -> high only: no edge has its reverse, no loops
    assert all(ei.shape[1] >= 20 and (ei[0] >= 8).any() and (ei[1] < 18).any() for ei in snaps)
    fixture('k3_directed', 30, 3, 16, 3, [(ei, None) for ei in snaps], seed=3)
    snaps = []
    for s, n in enumerate((30, 44, 25, 37)):
        ei = rand_edges(rng, 16, n, 0, 8, 0, 8)  # 64 ordered pairs for 25..44 draws: repeats
        loops = np.repeat(rng.integers(0, 16, 5), 2)[None].repeat(2, 0)  # every loop twice
        ei = np.concatenate([ei, loops, ei[:, :6]], axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        assert (ei[0] == ei[1]).sum() >= 10 and len(set(map(tuple, ei.T))) < ei.shape[1]
        snaps.append((ei, w(ei) if s % 2 else None))
    fixture('k4_loops_dups', 16, 6, 5, 4, snaps, seed=4)
    snaps = [rand_edges(rng, 18, n) for n in (25, 40, 30)]
    fixture('rw_lmax', 18, 4, 7, 3, [(ei, w(ei)) for ei in snaps], normalization='rw', lambda_max=2.5, seed=5)
    snaps = [both_ways(rand_edges(rng, 14, n)) for n in (12, 18, 15)]
    fixture('none_lmax', 14, 3, 4, 2, [(ei, w(ei) * 0.3) for ei in snaps], normalization=None, lambda_max=6.0, seed=6)
    fixture('empty_snapshot', 12, 4, 6, 2, [(both_ways(rand_edges(rng, 12, 14)), None), (np.zeros((2, 0), np.int64), None),
                                            (both_ways(rand_edges(rng, 12, 10)), None)], seed=7)  # fmt: skip
    fixture('nobias', 15, 5, 4, 2, [(both_ways(rand_edges(rng, 15, n)), None) for n in (16, 11, 19)], bias=False, seed=8)


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
