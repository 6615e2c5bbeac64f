"""CPU restatement of DyGFormer (neighbour co-occurrence counts and encoding, patching, transformer layers, per-side mean), written out
from the definitions for the tests: plain numpy / torch on the host, float64 where it is the checker (``float32(dt)`` is its input, as the
reference's Time2Vec takes it; everything after that in ``dtype``).  The product never imports this file."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

PAD = -1


def cooccurrence_counts(src_seq: np.ndarray, dst_seq: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """[P, L] id sequences -> ([P, L, 2], [P, L, 2]) int64: (occurrences in the own sequence, in the other one); pads zeroed."""
    src_seq, dst_seq = np.asarray(src_seq, dtype=np.int64), np.asarray(dst_seq, dtype=np.int64)
    out_s, out_d = np.zeros(src_seq.shape + (2,), dtype=np.int64), np.zeros(dst_seq.shape + (2,), dtype=np.int64)
    for p in range(src_seq.shape[0]):
        for mine, other, out in ((src_seq[p], dst_seq[p], out_s[p]), (dst_seq[p], src_seq[p], out_d[p])):
            ids, cnt = np.unique(mine, return_counts=True)
            own = dict(zip(ids.tolist(), cnt.tolist()))
            ids, cnt = np.unique(other, return_counts=True)
            cross = dict(zip(ids.tolist(), cnt.tolist()))
            for j, v in enumerate(mine.tolist()):
                if v != PAD:
                    out[j, 0], out[j, 1] = own[v], cross.get(v, 0)
    return out_s, out_d


def cooccurrence_encode(sd: Dict[str, torch.Tensor], prefix: str, counts: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[..., 2] counts -> [..., C]: the two-layer encoder on each count separately, summed."""
    g = lambda n: sd[prefix + n].to(dtype)
    h = F.relu(F.linear(counts.to(dtype).unsqueeze(-1), g('0.weight'), g('0.bias')))
    return F.linear(h, g('2.weight'), g('2.bias')).sum(dim=-2)


def transformer_layer(sd: Dict[str, torch.Tensor], prefix: str, x: torch.Tensor, num_heads: int, eps: float = 1e-5) -> torch.Tensor:
    """x [B, T, d]: x1 = x + MHA(LN0(x)); out = x1 + W2 gelu(W1 LN1(x1))."""
    g = lambda n: sd[prefix + n].to(x.dtype)
    B, T, d = x.shape
    dh = d // num_heads
    h = F.layer_norm(x, (d,), g('norm_layers.0.weight'), g('norm_layers.0.bias'), eps)
    qkv = F.linear(h, g('multi_head_attention.in_proj_weight'), g('multi_head_attention.in_proj_bias'))
    q, k, v = (t.reshape(B, T, num_heads, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
    att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1) @ v  # [B, H, T, dh]
    att = att.transpose(1, 2).reshape(B, T, d)
    x1 = x + F.linear(att, g('multi_head_attention.out_proj.weight'), g('multi_head_attention.out_proj.bias'))
    h = F.layer_norm(x1, (d,), g('norm_layers.1.weight'), g('norm_layers.1.bias'), eps)
    return x1 + F.linear(F.gelu(F.linear(h, g('linear_layers.0.weight'), g('linear_layers.0.bias'))), g('linear_layers.1.weight'), g('linear_layers.1.bias'))


def dygformer_forward(sd: Dict[str, torch.Tensor], patch_size: int, num_layers: int, num_heads: int, node_x, src, dst, edge_time, nbr_nids,
                      nbr_time, nbr_edge_x, dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    """DyGFormer on host tensors; rows [:P] of nbr_* belong to src, rows [P:2P] to dst."""
    g = lambda n: sd[n].to(dtype)
    P = src.numel()
    seeds = torch.cat([src.reshape(-1), dst.reshape(-1)]).long()
    ids = torch.cat([seeds[:, None], nbr_nids[: 2 * P].long()], dim=1)  # [2P, L]
    L = ids.shape[1]
    valid = (ids != PAD).unsqueeze(-1)
    node = node_x.to(dtype)[ids.clamp(min=0)] * valid
    ex = nbr_edge_x[: 2 * P].to(dtype)
    edge = torch.cat([ex.new_zeros((2 * P, 1, ex.shape[2])), ex], dim=1)
    t = torch.cat([edge_time.reshape(-1), edge_time.reshape(-1)]).long()
    dt = torch.cat([t.new_zeros((2 * P, 1)), t[:, None] - nbr_time[: 2 * P].long()], dim=1).to(torch.float32).to(dtype).unsqueeze(-1)
    time = torch.cos(F.linear(dt, g('time_encoder.w.weight'), g('time_encoder.w.bias'))) * valid
    cs, cd = cooccurrence_counts(ids[:P].numpy(), ids[P:].numpy())
    co = cooccurrence_encode(sd, 'co_occurrence_encoder.neighbor_co_occurrence_encoder.', torch.from_numpy(np.concatenate([cs, cd])), dtype)
    Np = L // patch_size
    chans = []
    for name, f in (('node', node), ('edge', edge), ('time', time), ('neighbor_co_occurrence', co)):
        chans.append(F.linear(f.reshape(2 * P, Np, -1), g(f'projection_layer.{name}.weight'), g(f'projection_layer.{name}.bias')))
    tok = torch.cat(chans, dim=2)
    z = torch.cat([tok[:P], tok[P:]], dim=1)
    for i in range(num_layers):
        z = transformer_layer(sd, f'transformers.{i}.', z, num_heads)
    out = lambda m: F.linear(m, g('output_layer.weight'), g('output_layer.bias'))
    return out(z[:, :Np].mean(dim=1)), out(z[:, Np:].mean(dim=1))


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


def hashed_state_dict(shapes: Dict[str, list], seed: int) -> Dict[str, torch.Tensor]:
    """A state_dict of the given shapes: matrices uniform in +-1 / sqrt(fan_in), vectors in +-0.1, LayerNorm weights 1 +- 0.1, Time2Vec's
    frequencies as Time2Vec initialises them."""
    out = {}
    for i, (name, shape) in enumerate(shapes.items()):
        n = int(np.prod(shape))
        u = hashed_uniform(n, seed * 1000 + i).reshape(shape)
        if name == 'time_encoder.w.weight':
            v = (1 / 10 ** np.linspace(0, 9, shape[0])).reshape(shape).astype(np.float32)
        elif len(shape) == 2:
            v = u / np.float32(math.sqrt(shape[1]))
        elif 'norm_layers' in name and name.endswith('weight'):
            v = np.float32(1.0) + np.float32(0.1) * u
        else:
            v = np.float32(0.1) * u
        out[name] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return out
