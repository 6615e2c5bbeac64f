"""The decoders restated from their definitions, on the CPU, in float64 (the yardstick) or float32 on request.

LinkPredictor: ``model(merge(z_src, z_dst)).view(-1)`` with ``merge`` the concatenation or ``lin_src(z_src) + lin_dst(z_dst)``;
NodePredictor: ``model(z)``; GraphPredictor: ``model(pool(z))`` with ``pool`` the column mean or sum; ``model`` is Linear, ReLU, ...,
Linear (tgm/nn/decoder/{link,node,graph}proppred.py, tgm/nn/modules/aggregation.py).  Nothing here imports the product or the reference;
the fixtures tests/golden/g26_decoder_*.npz were recorded by running the reference's classes (tests/golden/make_golden_decoders.py).
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, List, Tuple

import numpy as np
import torch
from torch import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# name -> (kind, constructor arguments, merge / pooling, rows)
CASES = {
    'link_concat_172_64': ('link', dict(node_dim=172, hidden_dim=64), 'concat', 65),
    'link_concat_100_100': ('link', dict(node_dim=100, hidden_dim=100), 'concat', 33),
    'link_concat_deep': ('link', dict(node_dim=5, hidden_dim=7, nlayers=5, out_dim=3), 'concat', 9),
    'link_concat_one_row': ('link', dict(node_dim=172, hidden_dim=64), 'concat', 1),
    'link_sum_128': ('link', dict(node_dim=128, hidden_dim=64), 'sum', 65),
    'link_sum_deep': ('link', dict(node_dim=5, hidden_dim=33, nlayers=3), 'sum', 9),
    'node_100': ('node', dict(in_dim=100, hidden_dim=64, out_dim=10), None, 70),
    'node_deep': ('node', dict(in_dim=7, hidden_dim=33, nlayers=4, out_dim=1), None, 9),
    'graph_mean_41': ('graph', dict(in_dim=128, hidden_dim=128), 'mean', 41),
    'graph_sum_41': ('graph', dict(in_dim=128, hidden_dim=128), 'sum', 41),
    'graph_mean_1': ('graph', dict(in_dim=128, hidden_dim=128), 'mean', 1),
}
EXPECTED_FIXTURES = sorted(CASES)
RTOL = 1e-5


def rel_err(got, ref) -> float:
    """max |got - ref| / max(1, |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def close(got, ref, tag) -> None:
    """1e-5 of max(1, |ref|)"""
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    worst = rel_err(got, ref) / RTOL
    assert worst <= 1.0, f'{tag}: {worst:.2f}x the 1e-5 bound'


def expected_keys(kind: str, kw: dict, op) -> Dict[str, tuple]:
    """The reference's ``state_dict``: name -> shape."""
    H, out, n = kw.get('hidden_dim', 64), kw.get('out_dim', 1), max(kw.get('nlayers', 2), 2)
    dim = kw['node_dim'] if kind == 'link' else kw['in_dim']
    want = {}
    if kind == 'link' and op == 'sum':
        for side in ('src', 'dst'):
            want[f'merge.lin_{side}.weight'], want[f'merge.lin_{side}.bias'] = (dim, dim), (dim,)
    widths = [2 * dim if op == 'concat' else dim] + [H] * (n - 1) + [out]
    for i in range(n):
        want[f'model.{2 * i}.weight'], want[f'model.{2 * i}.bias'] = (widths[i + 1], widths[i]), (widths[i + 1],)
    return want


def mlp(sd: Dict[str, Tensor], x: Tensor) -> Tensor:
    n = len([k for k in sd if k.startswith('model.') and k.endswith('.weight')])
    for i in range(n):
        x = x @ sd[f'model.{2 * i}.weight'].to(x.dtype).t() + sd[f'model.{2 * i}.bias'].to(x.dtype)
        if i < n - 1:
            x = torch.relu(x)
    return x


def link(sd, op: str, z_src, z_dst, dtype=torch.float64) -> Tensor:
    a, b = torch.as_tensor(z_src).to(dtype), torch.as_tensor(z_dst).to(dtype)
    if op == 'concat':
        h = torch.cat((a, b), dim=1)
    else:
        w = lambda k: sd[k].to(dtype)
        h = (a @ w('merge.lin_src.weight').t() + w('merge.lin_src.bias')) + (b @ w('merge.lin_dst.weight').t() + w('merge.lin_dst.bias'))
    return mlp(sd, h).reshape(-1)


def node(sd, z, dtype=torch.float64) -> Tensor:
    return mlp(sd, torch.as_tensor(z).to(dtype))


def graph(sd, op: str, z, dtype=torch.float64) -> Tensor:
    z = torch.as_tensor(z).to(dtype)
    return mlp(sd, z.mean(dim=0) if op == 'mean' else z.sum(dim=0))


def restate(meta: dict, sd, inputs: Dict[str, Tensor], dtype=torch.float64) -> Tensor:
    if meta['kind'] == 'link':
        return link(sd, meta['op'], inputs['z_src'], inputs['z_dst'], dtype)
    if meta['kind'] == 'node':
        return node(sd, inputs['z'], dtype)
    return graph(sd, meta['op'], inputs['z'], dtype)


def fixture_names() -> List[str]:
    return sorted(os.path.basename(p)[len('g26_decoder_') : -len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'g26_decoder_*.npz')))


def load_fixture(name: str) -> Tuple[dict, Dict[str, Tensor], Dict[str, Tensor], Tensor]:
    """(meta, state_dict, inputs, the reference's output)"""
    with np.load(os.path.join(GOLDEN, f'g26_decoder_{name}.npz')) as f:
        meta = json.loads(bytes(f['meta']).decode())
        sd = {k[2:]: torch.from_numpy(f[k]) for k in meta['keys']}  # the reference's key order
        inputs = {k: torch.from_numpy(f[k]) for k in ('z_src', 'z_dst', 'z') if k in f.files}
        return meta, sd, inputs, torch.from_numpy(f['out'])


def one_vs_many_loop(decoder, z: Tensor, src_idx: Tensor, dst_idx: Tensor, negatives) -> List[Tensor]:
    """The evaluation loop of the reference's examples (examples/linkproppred/tgat.py:115-127): one decoder call per positive edge."""
    out = []
    for b in range(src_idx.numel()):
        dst_ids = torch.cat([dst_idx[b].reshape(1).long(), negatives[b].reshape(-1).long()])
        src_ids = src_idx[b].long().repeat(len(dst_ids))
        out.append(decoder(z[src_ids], z[dst_ids]))
    return out
