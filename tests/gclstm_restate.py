"""ChebConv and the GCLSTM cell restated from their definitions, on the CPU, in float64 (the yardstick) or float32 on request.

ChebConv: the published definition of ``torch_geometric.nn.ChebConv`` -- ``get_laplacian`` (self loops dropped, degree over the SOURCE
index, 'sym' / 'rw' / None), the scaling ``2 L / lambda_max - I``, aggregation at the DESTINATION, the recurrence
``Tx_k = 2 L_hat Tx_{k-1} - Tx_{k-2}``.  GCLSTM: the gate wiring of the reference's tgm/nn/encoder/gclstm.py:97-107, 165-227.
Nothing here imports the product or the reference; the fixtures tests/golden/g23_gclstm_*.npz were recorded by running the reference's
class (tests/golden/make_golden_gclstm.py).
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
GATES = ('i', 'f', 'c', 'o')
EXPECTED_FIXTURES = ['empty_snapshot', 'k1', 'k2_weighted', 'k3_directed', 'k4_loops_dups', 'nobias', 'none_lmax', 'rw_lmax']
RTOL = 1e-5


def expected_shapes(in_channels: int, out_channels: int, K: int, bias: bool = True) -> Dict[str, tuple]:
    """The reference's ``state_dict``: name -> shape."""
    want = {}
    for g in GATES:
        want[f'W_{g}'] = (in_channels, out_channels)
        want[f'b_{g}'] = (1, out_channels)
        for k in range(K):
            want[f'conv_{g}.lins.{k}.weight'] = (out_channels, out_channels)
        if bias:
            want[f'conv_{g}.bias'] = (out_channels,)
    return want


def rel_err(got, ref) -> float:
    """max |got - ref| / max(1, |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def close(got, ref, tag) -> None:
    """tests/test_tgcn_oracle_cpu.py's bar: 1e-5 of max(1, |ref|)."""
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    worst = ((got - ref).abs() / (RTOL * ref.abs().clamp(min=1.0))).max().item()
    assert worst <= 1.0, f'{tag}: {worst:.2f}x the 1e-5 bound'


def resolve_lambda_max(lambda_max, normalization) -> float:
    if lambda_max is None:
        if normalization != 'sym':
            raise ValueError('lambda_max is needed when the normalization is not symmetric')
        return 2.0
    if isinstance(lambda_max, Tensor):
        if lambda_max.numel() != 1:
            raise NotImplementedError('one lambda_max per graph of a batch')
        return float(lambda_max.reshape(()).item())
    return float(lambda_max)


def scaled_laplacian(edge_index, edge_weight, N: int, normalization, lambda_max, dtype=torch.float64) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(row, col, m, d): the off-diagonal entries m_e of L_hat (at [col_e, row_e] of the operator applied below) and its diagonal d."""
    assert normalization in (None, 'sym', 'rw'), normalization
    ei = torch.as_tensor(edge_index).to(torch.int64)
    row, col = ei[0], ei[1]
    w = torch.ones(row.numel(), dtype=dtype) if edge_weight is None else torch.as_tensor(edge_weight).to(dtype).reshape(-1)
    lmax = torch.tensor(resolve_lambda_max(lambda_max, normalization), dtype=dtype)
    keep = row != col
    row, col, w = row[keep], col[keep], w[keep]
    deg = torch.zeros(N, dtype=dtype).index_add_(0, row, w)
    inf = float('inf')
    if normalization == 'sym':
        dis = deg.pow(-0.5)
        dis = dis.masked_fill(dis == inf, 0)
        m, d = -(dis[row] * w * dis[col]), torch.ones(N, dtype=dtype)
    elif normalization == 'rw':
        dinv = 1.0 / deg
        dinv = dinv.masked_fill(dinv == inf, 0)
        m, d = -(dinv[row] * w), torch.ones(N, dtype=dtype)
    else:
        m, d = -w, deg
    m = (2.0 * m) / lmax
    m = m.masked_fill(m == inf, 0)
    d = (2.0 * d) / lmax
    d = d.masked_fill(d == inf, 0) - 1.0
    return row, col, m, d


def propagate(lap, t: Tensor) -> Tensor:
    row, col, m, d = lap
    out = d.unsqueeze(1) * t
    if row.numel():
        out = out.index_add(0, col, m.unsqueeze(1) * t[row])
    return out


def cheb_basis(lap, x: Tensor, K: int) -> List[Tensor]:
    tx = [x]
    if K > 1:
        tx.append(propagate(lap, x))
    for _ in range(2, K):
        tx.append(2.0 * propagate(lap, tx[-1]) - tx[-2])
    return tx


def cheb_conv(weights: List[Tensor], bias: Optional[Tensor], x, edge_index, edge_weight=None, normalization='sym', lambda_max=None,
              dtype=torch.float64) -> Tensor:  # fmt: skip
    """weights: ``lins.{k}.weight`` [out, in], k < K."""
    x = torch.as_tensor(x).to(dtype)
    lap = scaled_laplacian(edge_index, edge_weight, x.shape[0], normalization, lambda_max, dtype)
    tx = cheb_basis(lap, x, len(weights))
    out = tx[0] @ weights[0].to(dtype).t()
    for k in range(1, len(weights)):
        out = out + tx[k] @ weights[k].to(dtype).t()
    return out if bias is None else out + bias.to(dtype)


def cheb_conv_dense(weights: List[Tensor], bias: Optional[Tensor], x, edge_index, edge_weight=None, normalization='sym', lambda_max=None) -> Tensor:
    """The same through an explicit [N, N] matrix, float64: L_hat[i, j] = sum of m_e over the edges j -> i, plus the diagonal."""
    x = torch.as_tensor(x).to(torch.float64)
    N = x.shape[0]
    row, col, m, d = scaled_laplacian(edge_index, edge_weight, N, normalization, lambda_max)
    L = torch.diag(d)
    for e in range(row.numel()):
        L[col[e], row[e]] += m[e]
    tx = [x]
    if len(weights) > 1:
        tx.append(L @ x)
    for _ in range(2, len(weights)):
        tx.append(2.0 * (L @ tx[-1]) - tx[-2])
    out = sum(t @ w.to(torch.float64).t() for t, w in zip(tx, weights))
    return out if bias is None else out + bias.to(torch.float64)


def gclstm_forward(sd: Dict[str, Tensor], node_x, edge_index, edge_weight=None, H=None, C=None, lambda_max=None, normalization='sym',
                   dtype=torch.float64) -> Tuple[Tensor, Tensor]:  # fmt: skip
    """One step of the cell from a ``state_dict`` with the reference's keys (K and bias are read off the keys)."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(node_x).to(dtype)
    N, Co = x.shape[0], sd['W_i'].shape[1]
    K = sum(1 for k in sd if k.startswith('conv_i.lins.'))
    H = torch.zeros(N, Co, dtype=dtype) if H is None else torch.as_tensor(H).to(dtype)
    C = torch.zeros(N, Co, dtype=dtype) if C is None else torch.as_tensor(C).to(dtype)
    lap = scaled_laplacian(edge_index, edge_weight, N, normalization, lambda_max, dtype)
    tx = cheb_basis(lap, H, K)
    pre = {}
    for g in GATES:
        conv = tx[0] @ sd[f'conv_{g}.lins.0.weight'].t()
        for k in range(1, K):
            conv = conv + tx[k] @ sd[f'conv_{g}.lins.{k}.weight'].t()
        if f'conv_{g}.bias' in sd:
            conv = conv + sd[f'conv_{g}.bias']
        pre[g] = x @ sd[f'W_{g}'] + conv + sd[f'b_{g}']
    I, F, O = torch.sigmoid(pre['i']), torch.sigmoid(pre['f']), torch.sigmoid(pre['o'])
    C = F * C + I * torch.tanh(pre['c'])
    return O * torch.tanh(C), C


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def fixture_names() -> List[str]:
    return sorted(os.path.basename(p)[len('g23_gclstm_') : -4] for p in glob.glob(os.path.join(GOLDEN, 'g23_gclstm_*.npz')))


def load_fixture(name: str):
    """(meta, params, snapshots): meta holds in_channels, out_channels, K, normalization, bias, lambda_max, num_nodes; a snapshot is a dict
    with x, edge_index, edge_weight (or None) and the reference's H, C after it."""
    z = np.load(os.path.join(GOLDEN, f'g23_gclstm_{name}.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('p.')}
    snaps = []
    for s in range(meta['snapshots']):
        snaps.append(dict(x=torch.from_numpy(z[f'x{s}']), edge_index=torch.from_numpy(z[f'ei{s}']),
                          edge_weight=torch.from_numpy(z[f'ew{s}']) if f'ew{s}' in z.files else None,
                          H=torch.from_numpy(z[f'H{s}']), C=torch.from_numpy(z[f'C{s}'])))  # fmt: skip
    return meta, params, snaps


def replay(meta, snaps, step):
    """Run ``step(x, edge_index, edge_weight, H, C, lambda_max) -> (H, C)`` as a recurrence over the snapshots; yields (s, H, C)."""
    H = C = None
    for s, snap in enumerate(snaps):
        H, C = step(snap['x'], snap['edge_index'], snap['edge_weight'], H, C, meta['lambda_max'])
        yield s, H, C
