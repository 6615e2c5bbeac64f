"""CPU restatement of GraphMixer's time-gap hook and encoder (the reference keeps both in examples/linkproppred/graphmixer.py), written
out here from their definitions for the tests: plain numpy / torch on the host, float64 where it is the checker.  The product never
imports this file."""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

PAD = -1


def time_gap_window(times: np.ndarray, start_idx: int, end_idx: int, start_time: Optional[int], batch_min_time: int, time_gap: int):
    """Global event range [lb, ub) of the time-gap window of a batch over events [start_idx, end_idx) (end_idx nominal)."""
    lb = 0 if start_time is None else int(np.searchsorted(times, start_time, side='left'))
    ub = int(np.searchsorted(times, batch_min_time - 1, side='right'))
    lo_c, hi_c = max(end_idx - time_gap, 0), end_idx
    lb = max(lo_c, min(hi_c, lb))
    ub = max(lo_c, min(hi_c, ub))
    return lb, ub


def time_gap_lists(times: np.ndarray, edge_event: np.ndarray, src: np.ndarray, dst: np.ndarray, start_idx: int, end_idx: int,
                   start_time: Optional[int], batch_min_time: int, time_gap: int, seeds) -> List[List[int]]:  # fmt: skip
    """Every seed's time-gap neighbours: for each window edge (u, v) in stream order, v joins u's list and u joins v's."""
    lb, ub = time_gap_window(times, start_idx, end_idx, start_time, batch_min_time, time_gap)
    keep = (edge_event >= lb) & (edge_event < ub)
    nbrs: Dict[int, List[int]] = defaultdict(list)
    for u, v in zip(src[keep].tolist(), dst[keep].tolist()):
        nbrs[u].append(v)
        nbrs[v].append(u)
    return [list(nbrs.get(int(s), [])) for s in seeds]


def flatten(lists: List[List[int]]):
    """(values, offsets) of a list of lists."""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    vals = np.array([v for x in lists for v in x], dtype=np.int32)
    return vals, off


def unflatten(vals: np.ndarray, off: np.ndarray) -> List[List[int]]:
    return [vals[off[i] : off[i + 1]].tolist() for i in range(len(off) - 1)]


def hook_lists(nbr, lo, cnt) -> List[List[int]]:
    """The lists a TimeGapNeighborHook output stands for."""
    nbr, lo, cnt = (np.asarray(t.cpu() if hasattr(t, 'cpu') else t) for t in (nbr, lo, cnt))
    return [nbr[lo[i] : lo[i] + cnt[i]].tolist() for i in range(len(lo))]


def mixer_forward(sd: Dict[str, torch.Tensor], prefix: str, x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """One MLP-Mixer block, x [B, K, C]: token mixing (LayerNorm over K, Linear, GELU, Linear, residual), then channel mixing."""
    g = lambda n: sd[prefix + n].to(x.dtype)
    K, C = x.shape[1], x.shape[2]
    h = F.layer_norm(x.transpose(1, 2), (K,), g('token_norm.weight'), g('token_norm.bias'), eps)
    h = F.linear(F.gelu(F.linear(h, g('token_feedforward.ffn.0.weight'), g('token_feedforward.ffn.0.bias'))),
                 g('token_feedforward.ffn.3.weight'), g('token_feedforward.ffn.3.bias'))  # fmt: skip
    z = x + h.transpose(1, 2)
    h = F.layer_norm(z, (C,), g('channel_norm.weight'), g('channel_norm.bias'), eps)
    h = F.linear(F.gelu(F.linear(h, g('channel_feedforward.ffn.0.weight'), g('channel_feedforward.ffn.0.bias'))),
                 g('channel_feedforward.ffn.3.weight'), g('channel_feedforward.ffn.3.bias'))  # fmt: skip
    return z + h


def encoder_forward(sd: Dict[str, torch.Tensor], num_layers: int, nbr_edge_x, seed_times, nbr_edge_time, nbr_nids, seeds,
                    tg_lists: List[List[int]], node_feat, dtype=torch.float64) -> torch.Tensor:  # fmt: skip
    """GraphMixer's encoder on host tensors (seeds: cat(edge_src, edge_dst, neg)); ``dtype`` float64 = the checker."""
    g = lambda n: sd[n].to(dtype)
    dt = (seed_times[:, None].long() - nbr_edge_time.long()).to(torch.float32).to(dtype).unsqueeze(-1)
    tf = torch.cos(F.linear(dt, g('time_encoder.w.weight'), g('time_encoder.w.bias')))
    z = F.linear(torch.cat([nbr_edge_x.to(dtype), tf], dim=-1), g('projection_layer.weight'), g('projection_layer.bias'))
    for i in range(num_layers):
        z = mixer_forward(sd, f'mlp_mixers.{i}.', z)
    valid = (nbr_nids != PAD).to(dtype)
    z_link = (z * valid.unsqueeze(-1)).sum(dim=1) / valid.sum(dim=1, keepdim=True).clamp(min=1)
    x = node_feat.to(dtype)
    tg = torch.zeros((len(tg_lists), x.shape[1]), dtype=dtype)
    for i, lst in enumerate(tg_lists):
        if lst:
            tg[i] = x[torch.tensor(lst, dtype=torch.long)].mean(dim=0)
    z_node = tg + x[seeds.long()]
    return F.linear(torch.cat([z_link, z_node], dim=1), g('output_layer.weight'), g('output_layer.bias'))


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max(1, |ref|)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max()) if ref.numel() else 0.0
