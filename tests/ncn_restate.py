"""NCNPredictor (the common-neighbour decoder of TNCN) restated densely in float64, in this project's words; the CPU and GPU tests and the
fixture generator share it.

    A[a, b]   how often (a, b) or (b, a) occurs in edge_index (a self-loop counts twice)
    R_i[r]    A[tar_i[r]] where r is the LAST position of the value tar_i[r] in tar_i, else a zero row ('last'; 'all': every row)
    I_i[r]    the same rule on the identity matrix
    W[r, n]   exp(-(float32(edge_time[r] - last_update[n]) / 10000)) -- the float32 recipe, then carried in float64 -- or 1
    k = 2     cn = ((R_i o R_j) o W) x
    k = 4     cn = [((I_i o R_j) o W) x | ((R_i o I_j) o W) x | ((R_i o R_j) o W) x]
    xs        [x[tar_i] * x[tar_j] | cn]; the reference's xs.relu() discards its result (relu_xs=True restates what it would have done)
    out       Linear(relu(Linear(xs))).view(-1)
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F


def _t(v, dtype=None) -> torch.Tensor:
    t = torch.as_tensor(v).detach().cpu() if not (isinstance(v, torch.Tensor) and v.requires_grad) else v
    return t if dtype is None else t.to(dtype)


def dense_adjacency(num_nodes: int, edge_index, dtype=torch.float64) -> torch.Tensor:
    ei = _t(edge_index, torch.int64)
    A = torch.zeros((num_nodes, num_nodes), dtype=dtype)
    if ei.shape[1]:
        ones = torch.ones(ei.shape[1], dtype=dtype)
        A.index_put_((ei[0], ei[1]), ones, accumulate=True)
        A.index_put_((ei[1], ei[0]), ones, accumulate=True)
    return A


def kept_rows(tar: torch.Tensor, duplicate_targets: str) -> torch.Tensor:
    """[B] bool: does position r keep its row?"""
    B = tar.numel()
    if duplicate_targets == 'all':
        return torch.ones(B, dtype=torch.bool)
    last = {}
    for r, v in enumerate(tar.tolist()):
        last[v] = r
    return torch.tensor([last[v] == r for r, v in enumerate(tar.tolist())], dtype=torch.bool)


def decay_weights(last_update, edge_time, dtype=torch.float64) -> torch.Tensor:
    lu, et = _t(last_update, torch.int64).reshape(-1), _t(edge_time, torch.int64).reshape(-1)
    gap = (et[:, None] - lu[None, :]).to(torch.float32) / torch.tensor(10000.0, dtype=torch.float32)
    return torch.exp(-gap.to(dtype))  # the argument is the float32 one; the exponential is taken exactly


def cn_emb(x, edge_index, tar_ei, k: int, last_update=None, edge_time=None, duplicate_targets: str = 'last', dtype=torch.float64) -> torch.Tensor:
    x = _t(x, dtype)
    N = x.shape[0]
    tar = _t(tar_ei, torch.int64)
    ti, tj = tar[0], tar[1]
    A = dense_adjacency(N, edge_index, dtype)
    eye = torch.eye(N, dtype=dtype)
    ki, kj = kept_rows(ti, duplicate_targets).to(dtype)[:, None], kept_rows(tj, duplicate_targets).to(dtype)[:, None]
    Ri, Rj, Ii, Ij = A[ti] * ki, A[tj] * kj, eye[ti] * ki, eye[tj] * kj
    W = 1.0 if last_update is None else decay_weights(last_update, edge_time, dtype)
    if k == 2:
        blocks = [Ri * Rj]
    elif k == 4:
        blocks = [Ii * Rj, Ri * Ij, Ri * Rj]
    else:
        raise NotImplementedError(f'k = {k}')
    return torch.cat([(b * W) @ x for b in blocks], dim=-1)


def forward(sd: Dict[str, torch.Tensor], x, edge_index, tar_ei, k: int, last_update=None, edge_time=None, duplicate_targets: str = 'last',
            relu_xs: bool = False, dtype=torch.float64) -> torch.Tensor:
    x = _t(x, dtype)
    tar = _t(tar_ei, torch.int64)
    xs = torch.cat([x[tar[0]] * x[tar[1]], cn_emb(x, edge_index, tar, k, last_update, edge_time, duplicate_targets, dtype)], dim=-1)
    if relu_xs:
        xs = xs.relu()
    w = lambda n: sd[n].to(dtype) if not sd[n].requires_grad else sd[n]
    h = F.linear(xs, w('xsmlp.0.weight'), w('xsmlp.0.bias')).relu()
    return F.linear(h, w('xsmlp.2.weight'), w('xsmlp.2.bias')).reshape(-1)


def rel_err(got, ref) -> float:
    """max |got - ref| / max(1, |ref|)."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max()) if ref.numel() else 0.0


def hashed_uniform(n: int, seed: int) -> np.ndarray:
    """n reproducible float32 values in [-1, 1): a splitmix64 finaliser over (seed, index) -- integer arithmetic only, so the fixture of
    a model too large to store records a seed instead of its values."""
    with np.errstate(over='ignore'):
        v = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        v = (v ^ (v >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        v = (v ^ (v >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        v ^= v >> np.uint64(31)
    return ((v >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


def hashed_x(num_nodes: int, channels: int, seed: int) -> torch.Tensor:
    """Node embeddings in [-1, 1) from a seed."""
    return torch.from_numpy(hashed_uniform(num_nodes * channels, seed * 1000 + 999).reshape(num_nodes, channels).copy())


def hashed_state_dict(shapes: Dict[str, list], seed: int) -> Dict[str, torch.Tensor]:
    """A state_dict of the given shapes from a seed: matrices uniform in +-1 / sqrt(fan_in), vectors in +-0.1."""
    out = {}
    for i, (name, shape) in enumerate(shapes.items()):
        u = hashed_uniform(int(np.prod(shape)), seed * 1000 + i).reshape(shape)
        v = u / np.float32(math.sqrt(shape[1])) if len(shape) == 2 else np.float32(0.1) * u
        out[name] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return out


def fixture_state_dict(meta: dict, arrays: dict) -> Dict[str, torch.Tensor]:
    if 'weights_seed' in meta:
        return hashed_state_dict(meta['shapes'], meta['weights_seed'])
    return {k: torch.from_numpy(arrays[f'p_{k}']) for k in meta['state_dict_keys']}


def fixture_x(meta: dict, arrays: dict) -> torch.Tensor:
    if 'x_seed' in meta:
        return hashed_x(meta['N'], meta['C'], meta['x_seed'])
    return torch.from_numpy(arrays['x'])


def fixture_times(meta: dict, arrays: dict) -> tuple:
    if not meta['decay']:
        return None, None
    return torch.from_numpy(arrays['last_update']), torch.from_numpy(arrays['edge_time'])
