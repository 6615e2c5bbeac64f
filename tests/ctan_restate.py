"""CTAN restated for the tests: the encoder's arithmetic (tgm/nn/encoder/ctan.py with PyG 2.6.1's AntiSymmetricConv, TransformerConv(heads=1,
root_weight=False) and TimeEncoder from their published definitions) in torch on the CPU, float64 by default and evaluable in float32 -- the
float32 evaluation plays the role of the reference's own float32 error -- and ``CTANMemory`` with ``LastAggregator`` in numpy.

    rel_t = |last_update[edge_index[0]] - t|                   int64
    rel   = (rel_t - mean_delta_t) / std_delta_t               as torch evaluates it on an int64 tensor: float32, in EVERY evaluation
    enc   = cos(rel * time_enc.lin.weight[:, 0] + time_enc.lin.bias)
    e     = [msg | enc]
    x     = node_x enc_x.weight^T + enc_x.bias;   A = W - W^T - gamma I
    num_iters times:  phi_i = sum_j softmax_j(q_i . (k_j + We e_ij) / sqrt(M)) (v_j + We e_ij) over the edges j -> i (0 without any),
                      x = x + epsilon tanh(phi + x A^T + bias)
    return tanh(x)
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

KEYS = {
    'time_enc.lin.weight': lambda M, D, T, S: (T, 1), 'time_enc.lin.bias': lambda M, D, T, S: (T,),
    'enc_x.weight': lambda M, D, T, S: (M, M + S), 'enc_x.bias': lambda M, D, T, S: (M,),
    'aconv.W': lambda M, D, T, S: (M, M), 'aconv.bias': lambda M, D, T, S: (M,), 'aconv.eye': lambda M, D, T, S: (M, M),
    'aconv.phi.lin_key.weight': lambda M, D, T, S: (M, M), 'aconv.phi.lin_key.bias': lambda M, D, T, S: (M,),
    'aconv.phi.lin_query.weight': lambda M, D, T, S: (M, M), 'aconv.phi.lin_query.bias': lambda M, D, T, S: (M,),
    'aconv.phi.lin_value.weight': lambda M, D, T, S: (M, M), 'aconv.phi.lin_value.bias': lambda M, D, T, S: (M,),
    'aconv.phi.lin_edge.weight': lambda M, D, T, S: (M, D + T),
}  # fmt: skip
PARAMS = [k for k in KEYS if k != 'aconv.eye']


def expected_shapes(edge_dim: int, memory_dim: int, time_dim: int, node_dim: int) -> dict:
    return {k: f(memory_dim, edge_dim, time_dim, node_dim) for k, f in KEYS.items()}


def ctan_forward(p: dict, node_x, last_update, edge_index, t, msg, num_iters=1, mean_delta_t=0.0, std_delta_t=1.0, epsilon=0.1, gamma=0.1,
                 dtype=torch.float64, use_abs: bool = True, swap_edge_blocks: bool = False) -> torch.Tensor:  # fmt: skip
    """p: the state_dict (CPU tensors; leaves that require grad are differentiated through).  use_abs=False and swap_edge_blocks=True are
    deliberately WRONG variants (no |.| on the time difference; lin_edge's column blocks as if the edge features were [enc | msg]) that
    the tests show to differ."""
    c = lambda v: v.to(dtype)
    src, tgt = edge_index[0].long(), edge_index[1].long()
    rel_t = last_update.long()[src] - t.long()
    if use_abs:
        rel_t = rel_t.abs()
    rel = ((rel_t - mean_delta_t) / std_delta_t).to(torch.float32)  # float32 whatever `dtype`: the reference computes it so
    assert rel.dtype == torch.float32
    tw, tb = c(p['time_enc.lin.weight'])[:, 0], c(p['time_enc.lin.bias'])
    enc = torch.cos(c(rel)[:, None] * tw[None, :] + tb[None, :])
    msg = c(msg)
    D, T = msg.shape[1], tw.shape[0]
    We = c(p['aconv.phi.lin_edge.weight'])
    # swapped: the time part first, as TGN's layer has it -- lin_edge's first T columns then meet enc, its last D the message
    e_in = torch.cat([enc, msg], dim=-1) if swap_edge_blocks else torch.cat([msg, enc], dim=-1)
    x = c(node_x) @ c(p['enc_x.weight']).T + c(p['enc_x.bias'])
    U, M = x.shape
    W = c(p['aconv.W'])
    A = W - W.T - gamma * torch.eye(M, dtype=dtype)
    e = e_in @ We.T
    for _ in range(num_iters):
        q = x @ c(p['aconv.phi.lin_query.weight']).T + c(p['aconv.phi.lin_query.bias'])
        k = x @ c(p['aconv.phi.lin_key.weight']).T + c(p['aconv.phi.lin_key.bias'])
        v = x @ c(p['aconv.phi.lin_value.weight']).T + c(p['aconv.phi.lin_value.bias'])
        h = x @ A.T + c(p['aconv.bias'])
        if e.shape[0]:
            score = (q[tgt] * (k[src] + e)).sum(-1) / math.sqrt(M)
            top = torch.full((U,), -math.inf, dtype=dtype).scatter_reduce(0, tgt, score.detach(), 'amax')
            w = torch.exp(score - top[tgt])
            den = torch.zeros(U, dtype=dtype).index_add(0, tgt, w)
            h = h + torch.zeros(U, M, dtype=dtype).index_add(0, tgt, (w / den[tgt])[:, None] * (v[src] + e))
        x = x + epsilon * torch.tanh(h)
    return torch.tanh(x)


def rel_err(got, ref) -> float:
    """max |got - ref| / max(1, |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


class CTANMemoryRestated:
    """CTANMemory with LastAggregator: per node of cat[src, pos_dst] the embedding row of the LOWEST position among those with the largest
    float32(t), last_update = the exact int64 maximum; plain overwrites."""

    def __init__(self, num_nodes: int, memory_dim: int, init_time: int = 0) -> None:
        self.N, self.M, self.init_time = num_nodes, memory_dim, init_time
        self.memory = np.zeros((num_nodes, memory_dim), dtype=np.float32)
        self.last_update = np.full(num_nodes, init_time, dtype=np.int64)

    def reset_state(self) -> None:
        self.memory[:] = 0
        self.last_update[:] = self.init_time

    def winners(self, src, dst, t) -> dict:
        """node -> (winning position, exact maximal time)"""
        idx = np.concatenate([np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)])
        tt = np.concatenate([np.asarray(t, dtype=np.int64)] * 2)
        tf = tt.astype(np.float32)
        best = {}
        for p, (v, f, ti) in enumerate(zip(idx.tolist(), tf.tolist(), tt.tolist())):
            if v not in best:
                best[v] = [p, f, ti]
            else:
                b = best[v]
                if f > b[1]:
                    b[0], b[1] = p, f
                b[2] = max(b[2], ti)
        return {v: (b[0], b[2]) for v, b in best.items()}

    def update_state(self, src, dst, t, src_emb, dst_emb) -> None:
        emb = np.concatenate([np.asarray(src_emb, dtype=np.float32), np.asarray(dst_emb, dtype=np.float32)])
        assert emb.shape[0] >= 2 * len(src)
        for v, (p, tmax) in self.winners(src, dst, t).items():
            self.memory[v] = emb[p]
            self.last_update[v] = tmax


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, f'g22_ctanmem_{name}.npz'))
    return z, json.loads(bytes(z['meta']).decode())


def replay(z, meta, make, update, reset, state):
    """Drive a memory through the fixture's operations; after each, state() must equal the record bit for bit."""
    mem = make(meta['num_nodes'], meta['memory_dim'], meta['init_time'])
    u = 0
    for i, kind in enumerate(meta['ops']):
        if kind == 'reset':
            reset(mem)
        else:
            a, b = int(z['bounds'][u]), int(z['bounds'][u + 1])
            update(mem, z['src'][a:b], z['dst'][a:b], z['t'][a:b], z[f'src_emb{u}'], z[f'dst_emb{u}'])
            u += 1
        memory, last_update = state(mem)
        assert memory.dtype == np.float32 and last_update.dtype == np.int64
        assert np.array_equal(memory.view(np.int32), z['memory'][i].view(np.int32)), f'memory differs after operation {i} ({kind})'
        assert np.array_equal(last_update, z['last_update'][i]), f'last_update differs after operation {i} ({kind})'
