"""The backward of TPNet's encoder restated in float64, pure torch on the CPU, in the manner of ``graphmixer_bwd_restate.py``: written
out from the formulas with explicit masks, no autograd.  The new launches of ``csrc/tpnet_bwd.hip`` return values and, under the same
names with ``_m``, the same formula with every term replaced by its absolute value: a worst-case rounding bound for a float32 evaluation
is ``chain * 2^-24 * magnitude`` with ``chain`` from the helpers below (counted from the kernels).

The token block is ``graphmixer_bwd_restate.token_backward``: the forward's refined column mean is mathematically the mean.  What is new
is the per-sequence partial row (:func:`partial_rows`), the time rows (:func:`time_rows`), the mean backward and the chain
(:func:`forward` in plain torch, so float64 autograd can differentiate it; :func:`backward` as formulas, pinned to that in
``tests/test_tpnet_train_cpu.py``).  The chain returns values only: its float32 evaluation is held to the project's bar against float64,
not to a per-launch bound.  Nothing here imports the product.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
from torch import Tensor

import graphmixer_bwd_restate as gm
import tpnet_restate as tr
from graphmixer_bwd_restate import F64, LAYER_NAMES, layer_masks, token_backward  # noqa: F401  (re-exported for the tests)

PAD = -1
PART_NAMES = ('token_feedforward.ffn.3.weight', 'token_feedforward.ffn.0.weight', 'token_feedforward.ffn.3.bias', 'token_norm.bias',
              'token_norm.weight', 'token_feedforward.ffn.0.bias')  # fmt: skip  (the partial row's column order)


def part_floats(K: int, Ht: int) -> int:
    return 2 * K * Ht + 3 * K + Ht


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------
def part_chain(K: int, Ht: int, C: int) -> int:
    """the token block's chain into a column's value (``token_chain``), one product, and the C-term sum over the sequence's columns"""
    return gm.token_chain(K, Ht) + 1 + C


def part_colsum_chain(K: int, Ht: int, C: int, Q: int) -> int:
    """the partial row's chain plus the Q-term column sum (two stages: at most Q additions)"""
    return part_chain(K, Ht, C) + Q


def time_chain() -> int:
    """evaluated in double and rounded once: the rounding of the float32 inputs' product is all that is left; 1 + 8 as the house rule"""
    return 1 + 8


def mean_chain() -> int:
    """one division, plus 8"""
    return 1 + 8


# ---- the new launches ---------------------------------------------------------------------------------------------------------------------------
def partial_rows(P: List[Tensor], x: Tensor, dz1: Tensor, m0: Tensor, m1: Tensor, eps: float = 1e-5) -> Dict[str, Tensor]:
    """``tgmx_tpnet_token_backward`` on x, dz1 [Q, K, C]: dx, and part [Q, 2 K Ht + 3 K + Ht] = per sequence
    [ do^T hd | da^T xn | sum do | sum dxn | sum dxn x-hat | sum da ] over its C columns; the six gradients (``LAYER_NAMES`` names) are
    its column sums.  Magnitudes under ``*_m``."""
    Q, K, C = x.shape
    r = token_backward(P, x, dz1, m0, m1, eps)
    Ht = P[2].shape[0]

    def rows(t):
        do, xn, dxn, gxh, hd, da = t.view(Q, C, -1).split([K, K, K, K, Ht, Ht], dim=2)
        return torch.cat([torch.einsum('qck,qcj->qkj', do, hd).reshape(Q, -1), torch.einsum('qcj,qck->qjk', da, xn).reshape(Q, -1), do.sum(1), dxn.sum(1),
                          gxh.sum(1), da.sum(1)], dim=1)  # fmt: skip

    out = dict(dx=r['dx'], dx_m=r['dx_m'], part=rows(r['rows']), part_m=rows(r['rows_m']))
    for n in LAYER_NAMES[:6]:
        out[n], out[n + '_m'] = r[n], r[n + '_m']
    return out


def part_to_grads(colsum: Tensor, K: int, Ht: int) -> Dict[str, Tensor]:
    """The six gradients as views of a summed partial row (the layout ``tgmx_tpnet_backward`` writes ``d_tok`` in)."""
    KH = K * Ht
    sizes = [KH, KH, K, K, K, Ht]
    shapes = [(K, Ht), (Ht, K), (K,), (K,), (K,), (Ht,)]
    return {n: v.reshape(s) for n, v, s in zip(PART_NAMES, colsum.split(sizes), shapes)}


def time_rows(dtime: Tensor, lg: Tensor, pad: Tensor, tw: Tensor, tb: Tensor) -> Dict[str, Tensor]:
    """``tgmx_tpnet_time_backward``: rows [R, 2 dT] = [ -sin(w lg + b) d lg | -sin(w lg + b) d ], 0 on pad rows; dtime [R, dT], lg / pad [R]."""
    d, l = dtime.to(F64), lg.to(F64).unsqueeze(1)
    keep = (~pad).to(F64).unsqueeze(1)
    s = -torch.sin(l * tw.to(F64).view(1, -1) + tb.to(F64).view(1, -1)) * keep
    v = s * d
    return dict(rows=torch.cat([v * l, v], 1), rows_m=torch.cat([v.abs() * l.abs(), v.abs()], 1))


def mean_backward(g: Tensor, k: int) -> Tensor:
    """``tgmx_tpnet_mean_backward``: dz [Q k, C], dz[q k + j] = g[q] / k."""
    return (g.to(F64) / k).repeat_interleave(k, dim=0)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------
def _layer(sd, l: int, dtype) -> List[Tensor]:
    return [sd[f'mlp_mixers.{l}.{n}'].to(dtype) for n in LAYER_NAMES]


def forward(sd: Dict[str, Tensor], num_layers: int, rp: Optional[dict], node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x,
            masks: Optional[List[List[Tensor]]] = None, dtype=F64, keep: Optional[dict] = None):  # fmt: skip
    """``tpnet_restate.tpnet_forward`` with a layer's four dropout scales (``masks[l]``; None: all ones), differentiable by autograd in every
    parameter; ``keep`` receives what the saving forward keeps: feat, x0, per layer z and z1, lg, pad."""
    g = lambda n: sd[n].to(dtype)
    B = int(torch.as_tensor(src).numel())
    nids = nbr_nids[: 2 * B].long()
    Q, k = nids.shape
    pad = nids == PAD
    node = node_x.to(dtype)[nids].masked_fill(pad.unsqueeze(-1), 0.0)
    t2 = torch.cat([edge_time.reshape(-1), edge_time.reshape(-1)]).long()
    lg = torch.log((t2[:, None] - nbr_time[: 2 * B].long() + 1).to(dtype))
    time = torch.cos(lg.unsqueeze(-1) * g('time_encoder.w.weight').view(-1) + g('time_encoder.w.bias')).masked_fill(pad.unsqueeze(-1), 0.0)
    feats = [node, time, nbr_edge_x[: 2 * B].to(dtype)]
    raw = []
    if rp is not None:
        tables = [sd[f'random_projections.random_projections.{i}'].detach() for i in range(rp['num_layer'] + 1)]
        for ends in (src, dst):
            e2 = torch.as_tensor(ends).long().reshape(-1).repeat(2).repeat_interleave(k)
            f = tr.rp_features(tables, nids.reshape(-1), e2, rp['concat'], rp['scale'], dtype)
            raw.append(f)
            h = torch.relu(f @ g('random_projections.mlp.0.weight').T + g('random_projections.mlp.0.bias'))
            feats.append((h @ g('random_projections.mlp.2.weight').T + g('random_projections.mlp.2.bias')).reshape(Q, k, -1))
    x0 = torch.cat(feats, dim=2)
    hp = torch.relu(x0 @ g('projection_layer.0.weight').T + g('projection_layer.0.bias'))
    z = hp @ g('projection_layer.2.weight').T + g('projection_layer.2.bias')
    zs, z1s = [], []
    for l in range(num_layers):
        P = _layer(sd, l, dtype)
        m = masks[l] if masks is not None else gm.unit_masks(Q, k, z.shape[-1], P[2].shape[0], P[8].shape[0], dtype)
        kk = {}
        zs.append(z.detach())
        z = gm.mixer_forward(P, z, m, keep=kk)
        z1s.append(kk['z1'])
    if keep is not None:
        keep.update(feat=torch.cat(raw).detach() if raw else None, x0=x0.detach(), zs=zs, z1s=z1s, lg=lg.detach(), pad=pad)
    out = z.mean(dim=1)
    return out[:B], out[B:]


def backward(sd: Dict[str, Tensor], num_layers: int, dims: dict, kept: dict, g: Tensor, masks: Optional[List[List[Tensor]]] = None, dtype=F64,
             mags: Optional[dict] = None) -> Dict[str, Tensor]:  # fmt: skip
    """The launch list of ``tgmx_tpnet_backward`` as formulas: parameter name -> gradient.  g = [dz_src; dz_dst] [2B, E];
    dims: dict(dN, dT, dE, od).  ``mags`` receives the magnitudes of the mixers' gradients (``graphmixer_bwd_restate``'s): the scale of a
    gradient that is all cancellation, such as d token_norm.weight over the constant columns of an all-pad batch."""
    w = lambda n: sd[n].detach().to(dtype)
    x0, pad, lg = kept['x0'], kept['pad'], kept['lg']
    Q, k = pad.shape
    R, E = Q * k, g.shape[1]
    dN, dT, od = dims['dN'], dims['dT'], dims['od']
    base = dN + dT + dims['dE']
    res: Dict[str, Tensor] = {}
    gz = mean_backward(g.to(dtype), k).view(Q, k, E)
    gz_m = gz.abs()
    for l in range(num_layers - 1, -1, -1):
        P = [p.detach() for p in _layer(sd, l, dtype)]
        m = masks[l] if masks is not None else gm.unit_masks(Q, k, E, P[2].shape[0], P[8].shape[0], dtype)
        r = gm.mixer_backward(P, kept['zs'][l], kept['z1s'][l], gz, m, g_m=gz_m)
        for n in LAYER_NAMES:
            res[f'mlp_mixers.{l}.{n}'] = r[n]
            if mags is not None:
                mags[f'mlp_mixers.{l}.{n}'] = r[n + '_m']
        gz, gz_m = r['dx'], r['dx_m']
    f, x0f = gz.reshape(R, E), x0.reshape(R, -1)
    W0, b0, W2 = w('projection_layer.0.weight'), w('projection_layer.0.bias'), w('projection_layer.2.weight')
    hp = torch.relu(x0f @ W0.T + b0)
    res['projection_layer.2.weight'], res['projection_layer.2.bias'] = f.T @ hp, f.sum(0)
    dhp = (f @ W2) * (hp > 0)
    res['projection_layer.0.weight'], res['projection_layer.0.bias'] = dhp.T @ x0f, dhp.sum(0)
    if dT:
        tw, tb = w('time_encoder.w.weight'), w('time_encoder.w.bias')
        rows = time_rows(dhp @ W0[:, dN : dN + dT], lg.reshape(-1), pad.reshape(-1), tw, tb)['rows']
        res['time_encoder.w.weight'], res['time_encoder.w.bias'] = rows[:, :dT].sum(0).view(dT, 1), rows[:, dT:].sum(0)
    if od:
        V1, c1, V2 = w('random_projections.mlp.0.weight'), w('random_projections.mlp.0.bias'), w('random_projections.mlp.2.weight')
        dpf = torch.cat([dhp @ W0[:, base : base + od], dhp @ W0[:, base + od : base + 2 * od]])  # [2R, od]: block 0 over block 1
        feat = kept['feat']
        fh = torch.relu(feat @ V1.T + c1)
        res['random_projections.mlp.2.weight'], res['random_projections.mlp.2.bias'] = dpf.T @ fh, dpf.sum(0)
        dfh = (dpf @ V2) * (fh > 0)
        res['random_projections.mlp.0.weight'], res['random_projections.mlp.0.bias'] = dfh.T @ feat, dfh.sum(0)
    return res


def parse_mode(value: Optional[str], default: str = 'native') -> str:
    """``TGMX_TPNET_BWD`` as the product reads it: 'native', 'py' and 'torch' are themselves, anything else is the default."""
    return value if value in ('native', 'py', 'torch') else default
