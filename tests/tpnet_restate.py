"""CPU restatement of TPNet (https://arxiv.org/abs/2410.04013: temporal walk matrices kept as random projections, pair features, the
MLP-Mixer encoder over the recent neighbours), written out from the paper's definitions and the reference's observable behaviour for the
tests: plain torch on the host, float64 where it is the checker.  The product never imports this file.

State: tables P[0 .. L], each [N, dim], and a time ``now``.  A batch of edges (u_e, v_e, t_e), with next = t of the last edge:
    P[i] <- P[i] exp(-lam (next - now))^i                                           for i >= 1
    P[i][u_e] += P[i-1][v_e] exp(-lam (next - t_e)),  P[i][v_e] += P[i-1][u_e] exp(-lam (next - t_e))
where the P[i-1] on the right is the decayed table BEFORE the batch adds to it (levels are processed from L down to 1).
"""
from __future__ import annotations

import math
import re
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

PAD = -1


def rp_update(tables: List[torch.Tensor], now, src, dst, time, lam: float, dtype=torch.float64) -> Tuple[List[torch.Tensor], int]:
    """One batch; returns (new tables, next).  Rows are accumulated in batch order: all sources first, then all destinations."""
    src, dst, time = (torch.as_tensor(v).long().reshape(-1) for v in (src, dst, time))
    nxt = int(time[-1])
    w = torch.exp(-lam * (nxt - time).to(dtype)).unsqueeze(1)
    decay = math.exp(-lam * (nxt - float(now)))
    old = [tables[0].to(dtype)] + [tables[i].to(dtype) * torch.tensor(decay, dtype=dtype) ** i for i in range(1, len(tables))]
    new = [old[0]]
    for i in range(1, len(tables)):
        t = old[i].clone()
        t.index_add_(0, src, old[i - 1][dst] * w)
        t.index_add_(0, dst, old[i - 1][src] * w)
        new.append(t)
    return new, nxt


def rp_features(tables: List[torch.Tensor], a, b, concat: bool, scale: bool, dtype=torch.float64) -> torch.Tensor:
    """[P, (2L+2)^2] (the Gram matrix of a's rows stacked over b's) or [P, (L+1)^2] (a's rows against b's); a negative id indexes from the end."""
    a, b = torch.as_tensor(a).long().reshape(-1), torch.as_tensor(b).long().reshape(-1)
    ra = torch.stack([t.to(dtype)[a] for t in tables], dim=1)
    rb = torch.stack([t.to(dtype)[b] for t in tables], dim=1)
    if concat:
        r = torch.cat([ra, rb], dim=1)
        f = r @ r.transpose(1, 2)
    else:
        f = ra @ rb.transpose(1, 2)
    f = f.reshape(a.numel(), -1)
    return torch.log(f.clamp(min=0) + 1.0) if scale else f


def rp_forward(sd: Dict[str, torch.Tensor], prefix: str, num_layer: int, a, b, concat: bool, scale: bool, dtype=torch.float64) -> torch.Tensor:
    g = lambda n: sd[prefix + n].to(dtype)
    f = rp_features([sd[f'{prefix}random_projections.{i}'] for i in range(num_layer + 1)], a, b, concat, scale, dtype)
    return F.linear(F.relu(F.linear(f, g('mlp.0.weight'), g('mlp.0.bias'))), g('mlp.2.weight'), g('mlp.2.bias'))


def mixer_forward(sd: Dict[str, torch.Tensor], prefix: str, x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """One MLP-Mixer block, x [B, K, C]: token mixing (LayerNorm over K, Linear, GELU, Linear, residual), then channel mixing."""
    g = lambda n: sd[prefix + n].to(x.dtype)
    K, C = x.shape[1], x.shape[2]
    h = F.layer_norm(x.transpose(1, 2), (K,), g('token_norm.weight'), g('token_norm.bias'), eps)
    h = F.linear(F.gelu(F.linear(h, g('token_feedforward.ffn.0.weight'), g('token_feedforward.ffn.0.bias'))), g('token_feedforward.ffn.3.weight'),
                 g('token_feedforward.ffn.3.bias'))  # fmt: skip
    z = x + h.transpose(1, 2)
    h = F.layer_norm(z, (C,), g('channel_norm.weight'), g('channel_norm.bias'), eps)
    h = F.linear(F.gelu(F.linear(h, g('channel_feedforward.ffn.0.weight'), g('channel_feedforward.ffn.0.bias'))), g('channel_feedforward.ffn.3.weight'),
                 g('channel_feedforward.ffn.3.bias'))  # fmt: skip
    return z + h


def tpnet_tokens(sd, rp: Optional[dict], node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x, dtype=torch.float64) -> torch.Tensor:
    """[2B, k, d_N + d_T + d_E (+ 2 out_dim)]; rows [:B] of nbr_* belong to src, rows [B:2B] to dst.  rp: dict(num_layer, concat, scale)."""
    g = lambda n: sd[n].to(dtype)
    B = int(torch.as_tensor(src).numel())
    nids = nbr_nids[: 2 * B].long()
    k = nids.shape[1]
    pad = (nids == PAD).unsqueeze(-1)
    node = node_x.to(dtype)[nids].masked_fill(pad, 0.0)  # (-1 reads the last row, which is then zeroed)
    t2 = torch.cat([edge_time.reshape(-1), edge_time.reshape(-1)]).long()
    lg = torch.log((t2[:, None] - nbr_time[: 2 * B].long() + 1).to(dtype))
    time = torch.cos(F.linear(lg.unsqueeze(-1), g('time_encoder.w.weight'), g('time_encoder.w.bias'))).masked_fill(pad, 0.0)
    feats = [node, time, nbr_edge_x[: 2 * B].to(dtype)]
    if rp is not None:
        flat = nids.reshape(-1)  # pad slots index the last table row
        for ends in (src, dst):
            e2 = torch.as_tensor(ends).long().reshape(-1).repeat(2).repeat_interleave(k)
            feats.append(rp_forward(sd, 'random_projections.', rp['num_layer'], flat, e2, rp['concat'], rp['scale'], dtype).reshape(2 * B, k, -1))
    return torch.cat(feats, dim=2)


def tpnet_forward(sd: Dict[str, torch.Tensor], num_layers: int, rp: Optional[dict], node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x,
                  dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    """TPNet on host tensors.  Pad tokens are NOT zeroed after the projection (the reference discards that masked_fill's result)."""
    g = lambda n: sd[n].to(dtype)
    B = int(torch.as_tensor(src).numel())
    tok = tpnet_tokens(sd, rp, node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x, dtype)
    z = F.linear(F.relu(F.linear(tok, g('projection_layer.0.weight'), g('projection_layer.0.bias'))), g('projection_layer.2.weight'), g('projection_layer.2.bias'))
    for i in range(num_layers):
        z = mixer_forward(sd, f'mlp_mixers.{i}.', z)
    z = z.mean(dim=1)
    return z[:B], z[B:]


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max(1, |ref|)."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max()) if ref.numel() else 0.0


def hashed_uniform(n: int, seed: int) -> np.ndarray:
    """n reproducible float32 values in [-1, 1): a splitmix64 finaliser over (seed, index) -- integer arithmetic only, so the fixture of
    a model too large to store records a seed instead of its weights."""
    with np.errstate(over='ignore'):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return ((x >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


def hashed_state_dict(shapes: Dict[str, list], dtypes: Dict[str, str], seed: int) -> Dict[str, torch.Tensor]:
    """A state_dict of the given shapes: matrices uniform in +-1 / sqrt(fan_in) (the level-0 table: +- sqrt(3 / dim), unit-variance rows
    over dim; deeper tables: a tenth of that, non-negative), vectors in +-0.1, LayerNorm weights 1 +- 0.1, Time2Vec's frequencies as
    Time2Vec initialises them, integer entries (the two times) zero."""
    out = {}
    for i, (name, shape) in enumerate(shapes.items()):
        if dtypes[name] != 'float32':
            out[name] = torch.zeros(shape, dtype=getattr(torch, dtypes[name]))
            continue
        n = int(np.prod(shape))
        u = hashed_uniform(n, seed * 1000 + i).reshape(shape)
        if name == 'time_encoder.w.weight':
            v = (1 / 10 ** np.linspace(0, 9, shape[0])).reshape(shape).astype(np.float32)
        elif re.search(r'(^|\.)random_projections\.\d+$', name):
            level0 = name.endswith('.0')
            v = u * np.float32(math.sqrt(3.0 / shape[1])) if level0 else np.abs(u) * np.float32(0.1 * math.sqrt(3.0 / shape[1]))
        elif len(shape) == 2:
            v = u / np.float32(math.sqrt(shape[1]))
        elif 'norm' in name and name.endswith('weight'):
            v = np.float32(1.0) + np.float32(0.1) * u
        else:
            v = np.float32(0.1) * u
        out[name] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return out
