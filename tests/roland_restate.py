"""GCNConv and the ROLAND recurrence restated from their definitions, on the CPU, in float64 (the yardstick) or float32 on request.

GCNConv: the published definition of ``torch_geometric.nn.GCNConv`` -- ``gcn_norm`` with ``add_remaining_self_loops`` (an explicit self
loop replaces the fill value, the LAST of several on one node wins; degree over the DESTINATION index, loop weight included; repeated
edges each count; deg = 0 gives the factor 0), aggregation at the destination.  ROLAND: the wiring of the reference's
tgm/nn/encoder/roland.py:86-151 (two layers, relu, the update with the previous embeddings: tau blend, ``GRUCell`` or ``Linear`` on the
concatenation).  Nothing here imports the product or the reference; the fixtures tests/golden/g24_roland_*.npz were recorded by running
the reference's class (tests/golden/make_golden_roland.py).
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EXPECTED_FIXTURES = ['empty_snapshot', 'fixed_tau', 'gru', 'learnable', 'learnable_default', 'loops_dups_isolated', 'mlp', 'moving', 'odd_widths']
RTOL = 1e-5


def expected_shapes(input_channel: int, out_channel: int, update) -> Dict[str, tuple]:
    """The reference's ``state_dict``: name -> shape."""
    C = out_channel
    want = {'conv1.lin.weight': (C, input_channel), 'conv1.bias': (C,), 'conv2.lin.weight': (C, C), 'conv2.bias': (C,)}
    if update == 'learnable':
        want['tau'] = (1,)
    for l in (1, 2):
        if update == 'gru':
            want.update({f'gru{l}.weight_ih': (3 * C, C), f'gru{l}.weight_hh': (3 * C, C), f'gru{l}.bias_ih': (3 * C,), f'gru{l}.bias_hh': (3 * C,)})
        elif update == 'mlp':
            want.update({f'mlp{l}.weight': (C, 2 * C), f'mlp{l}.bias': (C,)})
    return want


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
    if ref.numel() == 0:
        return
    worst = ((got - ref).abs() / (RTOL * ref.abs().clamp(min=1.0))).max().item()
    assert worst <= 1.0, f'{tag}: {worst:.2f}x the 1e-5 bound'


def gcn_norm(edge_index, edge_weight, N: int, fill: float = 1.0, add_self_loops: bool = True, dtype=torch.float64):
    """(src, dst, m, diag): the off-diagonal entries m_e of A_hat (at [dst_e, src_e]) and its diagonal."""
    ei = torch.as_tensor(edge_index).to(torch.int64)
    src, dst = ei[0], ei[1]
    w = torch.ones(src.numel(), dtype=dtype) if edge_weight is None else torch.as_tensor(edge_weight).to(dtype).reshape(-1)
    lw = torch.zeros(N, dtype=dtype)
    if add_self_loops:
        lw = torch.full((N,), fill, dtype=dtype)
        for e in range(src.numel()):  # sequential: the last loop of a node wins
            if src[e] == dst[e]:
                lw[dst[e]] = w[e]
        keep = src != dst
        src, dst, w = src[keep], dst[keep], w[keep]
    deg = lw.clone().index_add_(0, dst, w)
    dinv = deg.pow(-0.5)
    dinv = dinv.masked_fill(dinv == float('inf'), 0)
    return src, dst, dinv[src] * w * dinv[dst], dinv * lw * dinv


def propagate(norm, t: Tensor) -> Tensor:
    src, dst, m, diag = norm
    out = diag.unsqueeze(1) * t
    if src.numel():
        out = out.index_add(0, dst, m.unsqueeze(1) * t[src])
    return out


def dense_adjacency(norm, N: int) -> Tensor:
    src, dst, m, diag = norm
    A = torch.diag(diag)
    for e in range(src.numel()):
        A[dst[e], src[e]] += m[e]
    return A


def gcn_conv(weight, bias, x, edge_index, edge_weight=None, fill: float = 1.0, add_self_loops: bool = True, dtype=torch.float64) -> Tensor:
    """weight: ``lin.weight`` [out, in]"""
    x = torch.as_tensor(x).to(dtype)
    norm = gcn_norm(edge_index, edge_weight, x.shape[0], fill, add_self_loops, dtype)
    out = propagate(norm, x @ torch.as_tensor(weight).to(dtype).t())
    return out if bias is None else out + torch.as_tensor(bias).to(dtype)


def epilogue(s: Tensor, mode: str, prev: Optional[Tensor] = None, tau=0.0) -> Tensor:
    """What tgmx_gcn_propagate's epilogue does to s = A_hat t + bias."""
    if mode == 'none':
        return s
    r = torch.relu(s)
    return r if mode == 'relu' else tau * prev.to(s.dtype) + (1 - tau) * r


def gru_cell(sd, l: int, h: Tensor, prev: Tensor) -> Tensor:
    """``torch.nn.GRUCell``: r, z from the sums, n = tanh(gi_n + r gh_n), h' = (1 - z) n + z prev."""
    gi = h @ sd[f'gru{l}.weight_ih'].t() + sd[f'gru{l}.bias_ih']
    gh = prev @ sd[f'gru{l}.weight_hh'].t() + sd[f'gru{l}.bias_hh']
    C = h.shape[1]
    r = torch.sigmoid(gi[:, :C] + gh[:, :C])
    z = torch.sigmoid(gi[:, C : 2 * C] + gh[:, C : 2 * C])
    n = torch.tanh(gi[:, 2 * C :] + r * gh[:, 2 * C :])
    return (1 - z) * n + z * prev


def roland_forward(sd: Dict[str, Tensor], update, node_x, edge_index, prev: List[Tensor], tau: float = 0.0, dtype=torch.float64) -> List[Tensor]:
    """One snapshot (eval mode, no dropout): ``prev`` the two previous embeddings, ``tau`` the blend weight ('learnable': read from sd)."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    h = torch.as_tensor(node_x).to(dtype)
    norm = gcn_norm(edge_index, None, h.shape[0], 1.0, True, dtype)
    if update == 'learnable':
        tau = sd['tau']
    out = []
    for l in (1, 2):
        h = torch.relu(propagate(norm, h @ sd[f'conv{l}.lin.weight'].t()) + sd[f'conv{l}.bias'])
        p = torch.as_tensor(prev[l - 1]).to(dtype)
        if update == 'gru':
            h = gru_cell(sd, l, h, p)
        elif update == 'mlp':
            h = torch.cat((h, p), dim=1) @ sd[f'mlp{l}.weight'].t() + sd[f'mlp{l}.bias']
        else:
            h = tau * p + (1 - tau) * h
        out.append(h)
    return out


def moving_tau(tau: float, num_current_edges, num_previous_edges) -> float:
    """'moving': float32(prev / (prev + cur)) when both counts are given, else the last value."""
    if num_current_edges is None or num_previous_edges is None:
        return tau
    return float(np.float32(num_previous_edges / (num_previous_edges + num_current_edges)))


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def fixture_names() -> List[str]:
    return sorted(os.path.basename(p)[len('g24_roland_') : -4] for p in glob.glob(os.path.join(GOLDEN, 'g24_roland_*.npz')))


def load_fixture(name: str):
    """(meta, params, snapshots): meta holds input_channel, out_channel, num_nodes, update, tau, snapshots; a snapshot is a dict with x,
    edge_index, counts (num_current_edges, num_previous_edges, each possibly None) and the reference's H0, H1 after it."""
    z = np.load(os.path.join(GOLDEN, f'g24_roland_{name}.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('p.')}
    snaps = []
    for s in range(meta['snapshots']):
        snaps.append(dict(x=torch.from_numpy(z[f'x{s}']), edge_index=torch.from_numpy(z[f'ei{s}']), counts=tuple(meta['counts'][s]),
                          H0=torch.from_numpy(z[f'H0_{s}']), H1=torch.from_numpy(z[f'H1_{s}'])))  # fmt: skip
    return meta, params, snaps


def replay(meta, snaps, step):
    """Run ``step(s, x, edge_index, prev, num_current_edges, num_previous_edges) -> [H0, H1]`` as a recurrence over the snapshots: the
    first call gets ``prev = None`` (the module's zeros), every later one the outputs of the call before.  Yields (s, [H0, H1])."""
    prev = None
    for s, snap in enumerate(snaps):
        prev = step(s, snap['x'], snap['edge_index'], prev, *snap['counts'])
        yield s, prev


def restated_replay(meta, params, snaps, dtype=torch.float64):
    """The restatement over a fixture's snapshots, with the module's state handling (zeros first, 'moving' tau kept between calls)."""
    N, C = meta['num_nodes'], meta['out_channel']
    state = {'tau': 0.0 if meta['update'] == 'moving' else float(np.float32(meta['tau']))}

    def step(s, x, ei, prev, cur, prv):
        if meta['update'] == 'moving':
            state['tau'] = moving_tau(state['tau'], cur, prv)
        prev = [torch.zeros(N, C, dtype=dtype), torch.zeros(N, C, dtype=dtype)] if prev is None else prev
        return roland_forward(params, meta['update'], x, ei, prev, state['tau'], dtype)

    return list(replay(meta, snaps, step))
