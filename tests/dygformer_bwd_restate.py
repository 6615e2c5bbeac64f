"""The backward of DyGFormer and of one of its transformer layers restated in float64, pure torch on the CPU, in the manner of
``graphmixer_bwd_restate.py``: written out from the formulas with explicit masks (the four dropout sites of a layer), no autograd.

The forward with masks (:func:`layer_forward`, :func:`encoder_forward`) is plain torch, so float64 autograd can differentiate it: the
backward formulas are pinned to that in ``tests/test_dygformer_train_cpu.py``, and with unit masks the forward is ``dygformer_restate``'s
(whose counts, co-occurrence encoder and hashed weights it reuses).  Dropout masks: ``oracle.dropout_ref.dropout_scale`` with stream
``first + 4 l + site`` and the element index the flat index in the site's tensor -- 0 attention probabilities [P, H, T, T], 1 attention
output [R, D], 2 FFN hidden [R, 4 D], 3 FFN output [R, D]; token row r = p T + i is row i of pair p.  Nothing here imports the product.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

import dygformer_restate as R
from oracle.dropout_ref import dropout_scale

PAD = -1
LAYER_NAMES = ('norm_layers.0.weight', 'norm_layers.0.bias', 'multi_head_attention.in_proj_weight', 'multi_head_attention.in_proj_bias',
               'multi_head_attention.out_proj.weight', 'multi_head_attention.out_proj.bias', 'norm_layers.1.weight', 'norm_layers.1.bias',
               'linear_layers.0.weight', 'linear_layers.0.bias', 'linear_layers.1.weight', 'linear_layers.1.bias')  # fmt: skip
CHANNELS = ('node', 'edge', 'time', 'neighbor_co_occurrence')
CO = 'co_occurrence_encoder.neighbor_co_occurrence_encoder.'


def site_masks(p: float, seed: int, first_stream: int, num_layers: int, B: int, H: int, T: int, D: int, dtype=torch.float64) -> Optional[List[List[Tensor]]]:
    """Per layer the four masks (scale 1 / (1 - p) or 0), None when dropout is off."""
    if not p:
        return None
    shapes = ((B, H, T, T), (B * T, D), (B * T, 4 * D), (B * T, D))
    out = []
    for l in range(num_layers):
        out.append([dropout_scale(p, seed, first_stream + 4 * l + s, (sh[0], int(np.prod(sh[1:])))).reshape(sh).to(dtype) for s, sh in enumerate(shapes)])
    return out


def gelu(a: Tensor) -> Tensor:
    return 0.5 * a * (1 + torch.erf(a / math.sqrt(2.0)))


def gelu_grad(a: Tensor) -> Tensor:
    """Phi(a) + a phi(a)"""
    return 0.5 * (1 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def _ln(x: Tensor, g: Tensor, b: Tensor, eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    return xh * g + b, xh, rstd


def ln_backward(dy: Tensor, xh: Tensor, rstd: Tensor, g: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, d gamma, d beta)"""
    dxh = dy * g
    dx = rstd * (dxh - dxh.mean(dim=-1, keepdim=True) - xh * (dxh * xh).mean(dim=-1, keepdim=True))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return dx, flat(dy * xh).sum(dim=0), flat(dy).sum(dim=0)


# ---- attention --------------------------------------------------------------------------------------------------------------------------------
def _heads(t: Tensor, H: int) -> Tensor:
    B, T, d = t.shape
    return t.reshape(B, T, H, d // H).transpose(1, 2)  # [B, H, T, dh]


def attention_forward(qkv: Tensor, H: int, mask: Optional[Tensor]) -> Tensor:
    """qkv [B, T, 3 d] -> [B, T, d]; mask [B, H, T, T] scales the normalised probabilities."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (_heads(t, H) for t in qkv.split(d, dim=-1))
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d // H), dim=-1)
    if mask is not None:
        P = P * mask
    return (P @ v).transpose(1, 2).reshape(B, T, d)


def attention_backward(qkv: Tensor, datt: Tensor, H: int, mask: Optional[Tensor]) -> Tensor:
    """dqkv [B, T, 3 d]:  dV = (P o m)^T dO,  dP = (dO V^T) o m,  dS = P o (dP - rowsum(dP o P)),  dQ = scale dS K,  dK = scale dS^T Q."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    scale = 1.0 / math.sqrt(d // H)
    q, k, v = (_heads(t, H) for t in qkv.split(d, dim=-1))
    dO = _heads(datt, H)
    P = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    m = torch.ones_like(P) if mask is None else mask
    dV = (P * m).transpose(-1, -2) @ dO
    dP = (dO @ v.transpose(-1, -2)) * m
    dS = P * (dP - (dP * P).sum(dim=-1, keepdim=True))
    dQ, dK = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q)
    back = lambda t: t.transpose(1, 2).reshape(B, T, d)
    return torch.cat([back(dQ), back(dK), back(dV)], dim=-1)


# ---- one layer --------------------------------------------------------------------------------------------------------------------------------
def _layer_cache(w: Dict[str, Tensor], x: Tensor, H: int, masks: Optional[List[Tensor]], eps: float) -> dict:
    B, T, d = x.shape
    m = [None] * 4 if masks is None else [masks[0], masks[1].reshape(B, T, d), masks[2].reshape(B, T, 4 * d), masks[3].reshape(B, T, d)]
    one = lambda t, k: t if m[k] is None else t * m[k]
    c = dict(m=m)
    c['y0'], c['xh0'], c['rstd0'] = _ln(x, w[LAYER_NAMES[0]], w[LAYER_NAMES[1]], eps)
    c['qkv'] = F.linear(c['y0'], w[LAYER_NAMES[2]], w[LAYER_NAMES[3]])
    c['att'] = attention_forward(c['qkv'], H, m[0])
    c['x1'] = x + one(F.linear(c['att'], w[LAYER_NAMES[4]], w[LAYER_NAMES[5]]), 1)
    c['y1'], c['xh1'], c['rstd1'] = _ln(c['x1'], w[LAYER_NAMES[6]], w[LAYER_NAMES[7]], eps)
    c['a'] = F.linear(c['y1'], w[LAYER_NAMES[8]], w[LAYER_NAMES[9]])
    c['hd'] = one(gelu(c['a']), 2)
    c['out'] = c['x1'] + one(F.linear(c['hd'], w[LAYER_NAMES[10]], w[LAYER_NAMES[11]]), 3)
    return c


def layer_weights(sd: Dict[str, Tensor], prefix: str, dtype) -> Dict[str, Tensor]:
    return {n: sd[prefix + n].to(dtype) for n in LAYER_NAMES}


def layer_forward(w: Dict[str, Tensor], x: Tensor, H: int, masks: Optional[List[Tensor]] = None, eps: float = 1e-5) -> Tensor:
    """x [B, T, d] -> [B, T, d]; ``w``: the twelve tensors under LAYER_NAMES; masks: the layer's four sites."""
    return _layer_cache(w, x, H, masks, eps)['out']


def layer_backward(w: Dict[str, Tensor], x: Tensor, g: Tensor, H: int, masks: Optional[List[Tensor]] = None, eps: float = 1e-5) -> Tuple[Tensor, Dict[str, Tensor]]:
    """(dx, the twelve gradients under LAYER_NAMES) given g = the gradient at the layer's output."""
    c = _layer_cache(w, x, H, masks, eps)
    m = c['m']
    one = lambda t, k: t if m[k] is None else t * m[k]
    flat = lambda t: t.reshape(-1, t.shape[-1])
    d: Dict[str, Tensor] = {}
    g3 = one(g, 3)
    d[LAYER_NAMES[10]], d[LAYER_NAMES[11]] = flat(g3).t() @ flat(c['hd']), flat(g3).sum(dim=0)
    da = one(g3 @ w[LAYER_NAMES[10]], 2) * gelu_grad(c['a'])
    d[LAYER_NAMES[8]], d[LAYER_NAMES[9]] = flat(da).t() @ flat(c['y1']), flat(da).sum(dim=0)
    du, d[LAYER_NAMES[6]], d[LAYER_NAMES[7]] = ln_backward(da @ w[LAYER_NAMES[8]], c['xh1'], c['rstd1'], w[LAYER_NAMES[6]])
    dx1 = g + du
    g1 = one(dx1, 1)
    d[LAYER_NAMES[4]], d[LAYER_NAMES[5]] = flat(g1).t() @ flat(c['att']), flat(g1).sum(dim=0)
    dqkv = attention_backward(c['qkv'], g1 @ w[LAYER_NAMES[4]], H, m[0])
    d[LAYER_NAMES[2]], d[LAYER_NAMES[3]] = flat(dqkv).t() @ flat(c['y0']), flat(dqkv).sum(dim=0)
    du, d[LAYER_NAMES[0]], d[LAYER_NAMES[1]] = ln_backward(dqkv @ w[LAYER_NAMES[2]], c['xh0'], c['rstd0'], w[LAYER_NAMES[0]])
    return dx1 + du, d


# ---- the tails ----------------------------------------------------------------------------------------------------------------------------------
def mean_backward(dmean: Tensor, P: int, Np: int) -> Tensor:
    """dmean [2 P, D] (sources first) -> dz [P, 2 Np, D]: every token of a side gets its side's gradient / Np."""
    D = dmean.shape[1]
    return torch.cat([dmean[:P, None, :].expand(P, Np, D), dmean[P:, None, :].expand(P, Np, D)], dim=1) / Np


def time_backward(dtime: Tensor, dt: Tensor, valid: Tensor, tw: Tensor, tb: Tensor) -> Tuple[Tensor, Tensor]:
    """dtime [2 P, L, dT], dt [2 P, L, 1], valid [2 P, L, 1] -> (d weight [dT, 1], d bias [dT]) of time = cos(dt w + b) valid."""
    gb = -torch.sin(dt * tw.reshape(1, 1, -1) + tb) * dtime * valid
    return (gb * dt).sum(dim=(0, 1)).reshape(-1, 1), gb.sum(dim=(0, 1))


def cooccurrence_backward(dfeat: Tensor, counts: Tensor, L: int, w1: Tensor, b1: Tensor, w2: Tensor) -> Dict[str, Tensor]:
    """dfeat [n, C], counts [n, 2] int64 -> the encoder's four gradients through its table over c = 0 .. L."""
    C = dfeat.shape[1]
    dtable = torch.zeros((L + 1, C), dtype=dfeat.dtype)
    dtable.index_add_(0, counts[:, 0], dfeat)
    dtable.index_add_(0, counts[:, 1], dfeat)
    c = torch.arange(L + 1, dtype=dfeat.dtype).reshape(-1, 1)
    pre = c * w1.reshape(1, -1) + b1
    r = pre.clamp(min=0)
    dh = (dtable @ w2) * (pre > 0)
    return {CO + '0.weight': (dh * c).sum(dim=0).reshape(-1, 1), CO + '0.bias': dh.sum(dim=0), CO + '2.weight': dtable.t() @ r, CO + '2.bias': dtable.sum(dim=0)}


def relu_margin(sd: Dict[str, Tensor], L: int) -> float:
    """min |w1 c + b1| over c = 0 .. L and all channels: the float64 and float32 ReLU masks of the table agree when this is well above
    float32's rounding of the expression."""
    c = torch.arange(L + 1, dtype=torch.float64).reshape(-1, 1)
    return float((c * sd[CO + '0.weight'].double().reshape(1, -1) + sd[CO + '0.bias'].double()).abs().min())


# ---- the whole encoder ------------------------------------------------------------------------------------------------------------------------
def _inputs(sd, node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x, dtype) -> dict:
    P = src.numel()
    seeds = torch.cat([src.reshape(-1), dst.reshape(-1)]).long()
    ids = torch.cat([seeds[:, None], nbr_nids[: 2 * P].long()], dim=1)
    valid = (ids != PAD).unsqueeze(-1)
    node = node_x.to(dtype)[ids.clamp(min=0)] * valid
    ex = nbr_edge_x[: 2 * P].to(dtype)
    edge = torch.cat([ex.new_zeros((2 * P, 1, ex.shape[2])), ex], dim=1)
    t = torch.cat([edge_time.reshape(-1), edge_time.reshape(-1)]).long()
    dt = torch.cat([t.new_zeros((2 * P, 1)), t[:, None] - nbr_time[: 2 * P].long()], dim=1).to(torch.float32).to(dtype).unsqueeze(-1)
    cs, cd = R.cooccurrence_counts(ids[:P].numpy(), ids[P:].numpy())
    counts = torch.from_numpy(np.concatenate([cs, cd]))  # [2 P, L, 2]
    return dict(P=P, L=ids.shape[1], valid=valid.to(dtype), node=node, edge=edge, dt=dt, counts=counts)


def encoder_forward(sd: Dict[str, Tensor], patch_size: int, num_layers: int, num_heads: int, node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x,
                    masks: Optional[List[List[Tensor]]] = None, dtype=torch.float64, keep: Optional[dict] = None) -> Tuple[Tensor, Tensor]:  # fmt: skip
    """``dygformer_restate.dygformer_forward`` with the dropout sites' masks (None: the same values).  ``sd`` may hold tensors that require
    grad.  keep: receives the intermediates the hand-written backward reads."""
    g = lambda n: sd[n].to(dtype)
    i = _inputs(sd, node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x, dtype)
    P, L = i['P'], i['L']
    time = torch.cos(F.linear(i['dt'], g('time_encoder.w.weight'), g('time_encoder.w.bias'))) * i['valid']
    co = R.cooccurrence_encode(sd, CO, i['counts'], dtype)
    Np = L // patch_size
    feats = [f.reshape(2 * P, Np, -1) for f in (i['node'], i['edge'], time, co)]
    tok = torch.cat([F.linear(f, g(f'projection_layer.{n}.weight'), g(f'projection_layer.{n}.bias')) for n, f in zip(CHANNELS, feats)], dim=2)
    z = torch.cat([tok[:P], tok[P:]], dim=1)
    xs = []
    for l in range(num_layers):
        xs.append(z)
        z = layer_forward(layer_weights(sd, f'transformers.{l}.', dtype), z, num_heads, None if masks is None else masks[l])
    means = torch.cat([z[:, :Np].mean(dim=1), z[:, Np:].mean(dim=1)], dim=0)
    out = F.linear(means, g('output_layer.weight'), g('output_layer.bias'))
    if keep is not None:
        keep.update(i, feats=feats, xs=xs, means=means, Np=Np)
    return out[:P], out[P:]


def encoder_backward(sd: Dict[str, Tensor], patch_size: int, num_layers: int, num_heads: int, node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x,
                     g_src: Tensor, g_dst: Tensor, masks: Optional[List[List[Tensor]]] = None, dtype=torch.float64) -> Dict[str, Tensor]:  # fmt: skip
    """Every parameter's gradient by hand, keyed as the state_dict: the output layer, the mean, the layers last first, the four projections,
    the time and co-occurrence tails."""
    k: dict = {}
    sdd = {n: v.detach().to(dtype) for n, v in sd.items()}
    with torch.no_grad():
        encoder_forward(sdd, patch_size, num_layers, num_heads, node_x, src, dst, edge_time, nbr_nids, nbr_time, nbr_edge_x, masks, dtype, keep=k)
        P, L, Np = k['P'], k['L'], k['Np']
        g = torch.cat([g_src, g_dst], dim=0).to(dtype)
        d: Dict[str, Tensor] = {'output_layer.weight': g.t() @ k['means'], 'output_layer.bias': g.sum(dim=0)}
        gz = mean_backward(g @ sdd['output_layer.weight'], P, Np)
        for l in range(num_layers - 1, -1, -1):
            gz, dl = layer_backward(layer_weights(sdd, f'transformers.{l}.', dtype), k['xs'][l], gz, num_heads, None if masks is None else masks[l])
            d.update({f'transformers.{l}.{n}': v for n, v in dl.items()})
        dtok = torch.cat([gz[:, :Np], gz[:, Np:]], dim=0)  # [2 P, Np, D], sources first
        C = sdd['projection_layer.node.bias'].numel()
        flat = lambda t: t.reshape(-1, t.shape[-1])
        dfeat = []
        for c, n in enumerate(CHANNELS):
            gc = dtok[:, :, c * C : (c + 1) * C]
            d[f'projection_layer.{n}.weight'], d[f'projection_layer.{n}.bias'] = flat(gc).t() @ flat(k['feats'][c]), flat(gc).sum(dim=0)
            dfeat.append((gc @ sdd[f'projection_layer.{n}.weight']).reshape(2 * P, L, -1))
        d['time_encoder.w.weight'], d['time_encoder.w.bias'] = time_backward(dfeat[2], k['dt'], k['valid'], sdd['time_encoder.w.weight'], sdd['time_encoder.w.bias'])
        d.update(cooccurrence_backward(flat(dfeat[3]), k['counts'].reshape(-1, 2), L, sdd[CO + '0.weight'], sdd[CO + '0.bias'], sdd[CO + '2.weight']))
    return d


def max_ratio(got: Tensor, ref: Tensor) -> float:
    """max |got - ref| / max |ref| (the project's gradient bar is on this figure); 0 for two all-zero tensors."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    top = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    return err / top if top > 0 else err
