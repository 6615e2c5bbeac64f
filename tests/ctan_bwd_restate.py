"""The backward of CTAN's encoder restated in float64 (or float32 on request), pure torch on the CPU, in the manner of
``gclstm_bwd_restate.py``: every block returns values and, under the same names with ``_m``, the same formula with every term replaced by
its absolute value.  A worst-case rounding bound for a float32 evaluation is ``chain * 2^-24 * magnitude`` with ``chain`` from the chain
helpers below (counted from ``csrc/ctan_bwd.hip``).

Magnitudes follow ``gclstm_bwd_restate``'s rules: a difference counts as the sum of its terms' magnitudes (``1 - t^2`` as ``1 + t^2``); a
function of a rounded value counts as its own value plus its derivative times the argument's magnitude (``tanh z`` as ``|tanh z| + (1 -
tanh^2 z) mag(z)``, ``sin a`` as ``|sin a| + mag(a)``).  A softmax weight is ``exp`` of a difference of two rounded scores over a sum of such:
it counts as ``alpha (1 + mag(score_e) + max over the segment of mag(score))``.

The blocks: :func:`target_pass` (``tgmx_ctan_attend_backward``), :func:`source_pass` (``tgmx_ctan_source_backward``),
:func:`edge_attr_backward` (``tgmx_ctan_edge_attr_backward``), :func:`antisym_grad` (``tgmx_ctan_antisym_grad``) and :func:`backward`
(``tgmx_ctan_backward``).  Nothing here imports the product or the reference; the forward is ``ctan_restate.ctan_forward``'s arithmetic.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

from oracle.tgat_bwd_ref import EPS, F64
from oracle.tgn_bwd_ref import TRANSCENDENTAL_OPS

SHORT, WAVES, WAVE = 16, 4, 64  # kCtanShort, kCtanWaves, the wave size
SEG_LENS = [0, 1, 16, 17, 64, 65, 1500, 3, 0, 130]
WIDTHS = [4, 5, 64, 100, 130, 256]


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------
def per_wave(n):
    """edges one wave walks of a segment of n: all of them up to kCtanShort, every fourth beyond (a number or a tensor)"""
    if torch.is_tensor(n):
        return torch.where(n > SHORT, (n + WAVES - 1) // WAVES, n)
    return (n + WAVES - 1) // WAVES if n > SHORT else n


def dot_chain(C: int) -> int:
    """a row dot product: one product and V - 1 fmas in the lane's own columns (V = ceil(C / 64)), six butterfly additions"""
    return (C + WAVE - 1) // WAVE + 6


def attend_chain(C: int, n):
    """float32 operations on the longest chain into an element of dq / d_eproj, plus 8, counted from ctan_attend_backward_kernel.
    Walk 1 per edge of the wave: the key sum (1), the dot product, the scale (1), then the running state -- expf (4), the product with corr
    and the fma (2); only the state's 6 are on the chain from edge to edge.  The merge: expf, a product and a sum per wave (4 + 2 each, 4
    waves).  phi = acc / l (1), z (1), tanhf (4), 1 - t^2 (2), eps g (..) (2), delta (a dot product).  Walk 2: the edge's score again (its
    dot product + 2), the subtraction, expf, the division (1 + 4 + 1), dalpha (a dot product), dalpha - delta, two products (3), and one fma
    per edge of the wave into dq; its merge adds 4."""
    d = dot_chain(C)
    walk1 = (1 + d + 1) + (TRANSCENDENTAL_OPS + 2) * per_wave(n) + WAVES * (TRANSCENDENTAL_OPS + 2)
    epilogue = 1 + 1 + TRANSCENDENTAL_OPS + 2 + 2 + d
    walk2 = (d + 2) + (1 + TRANSCENDENTAL_OPS + 1) + d + 3 + per_wave(n) + WAVES
    return walk1 + epilogue + walk2 + 8


def source_chain(n):
    """one fma per edge of the wave, the merge's 4 additions, plus 8 (ctan_source_backward_kernel)"""
    return per_wave(n) + WAVES + 8


def edge_attr_chain() -> int:
    """rel w + b (one fma), the sine (the range reduction's 2 and the polynomial's 4), the product with d_attr, the product with rel, plus 8"""
    return 1 + 2 + TRANSCENDENTAL_OPS + 1 + 1 + 8


def antisym_chain() -> int:
    """one subtraction, plus 8"""
    return 1 + 8


def backward_chain(U: int, E: int, M: int, in_ch: int, Wd: int, num_iters: int, longest_in: int, longest_out: int) -> int:
    """One figure for every gradient of the encoder: per iteration the target and source passes at the longest segments, the projection's
    sum over 4M columns and the weight gradients' over U rows (E for lin_edge / time_enc); the iterations chain through gx."""
    per_it = attend_chain(M, longest_in) + source_chain(longest_out) + 4 * M + M
    return 3 + num_iters * per_it + max(U, E, in_ch, Wd) + edge_attr_chain() + 8


# ---- the blocks ---------------------------------------------------------------------------------------------------------------------------------
def _segment_softmax(score: Tensor, tgt: Tensor, U: int):
    top = torch.full((U,), -math.inf, dtype=score.dtype).scatter_reduce(0, tgt, score, 'amax')
    w = torch.exp(score - top[tgt])
    den = torch.zeros(U, dtype=score.dtype).index_add(0, tgt, w)
    return w / den[tgt]


def target_pass(q, k, v, h4, ep, src, tgt, gx, scale: float, eps: float, dtype=F64, gx_m: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """q, k, v, h4, gx [U, C], ep [E, C], src / tgt [E] in [0, U):

        alpha_e = softmax over the edges into tgt_e of scale q_i . (k_j + ep_e);  phi_i = sum_e alpha_e (v_j + ep_e);  z = h4 + phi
        dz = eps gx (1 - tanh^2 z);  delta_i = dz_i . phi_i;  dalpha_e = dz_i . (v_j + ep_e);  s_e = scale alpha_e (dalpha_e - delta_i)
        dq_i = sum_e s_e (k_j + ep_e);  de_e = s_e q_i + alpha_e dz_i

    Returns dz, dq, alpha, s, de and their magnitudes (``*_m``)."""
    q, k, v, h4, ep, gx = (t.to(dtype) for t in (q, k, v, h4, ep, gx))
    gx_m = gx.abs() if gx_m is None else gx_m.to(dtype)
    U = q.shape[0]
    kk, vv = k[src] + ep, v[src] + ep
    kk_m, vv_m = k[src].abs() + ep.abs(), v[src].abs() + ep.abs()
    score, score_m = (q[tgt] * kk).sum(-1) * scale, (q[tgt].abs() * kk_m).sum(-1) * scale
    alpha = _segment_softmax(score, tgt, U)
    seg_m = torch.zeros(U, dtype=dtype).scatter_reduce(0, tgt, score_m, 'amax')
    alpha_m = alpha * (1 + score_m + seg_m[tgt])
    zero = torch.zeros_like(q)
    phi, phi_m = zero.index_add(0, tgt, alpha[:, None] * vv), zero.index_add(0, tgt, alpha_m[:, None] * vv_m)
    tz = torch.tanh(h4 + phi)
    tz_m = tz.abs() + (1 - tz * tz) * (h4.abs() + phi_m)
    dz, dz_m = eps * gx * (1 - tz * tz), eps * gx_m * (1 + tz_m * tz_m)
    delta, delta_m = (dz * phi).sum(-1), (dz_m * phi_m).sum(-1)
    dal, dal_m = (dz[tgt] * vv).sum(-1), (dz_m[tgt] * vv_m).sum(-1)
    s, s_m = scale * alpha * (dal - delta[tgt]), scale * alpha_m * (dal_m + delta_m[tgt])
    dq, dq_m = zero.index_add(0, tgt, s[:, None] * kk), zero.index_add(0, tgt, s_m[:, None] * kk_m)
    de, de_m = s[:, None] * q[tgt] + alpha[:, None] * dz[tgt], s_m[:, None] * q[tgt].abs() + alpha_m[:, None] * dz_m[tgt]
    return dict(dz=dz, dq=dq, alpha=alpha, s=s, de=de, dz_m=dz_m, dq_m=dq_m, alpha_m=alpha_m, s_m=s_m, de_m=de_m)


def source_pass(q, dz, src, tgt, alpha, s, dtype=F64, dz_m=None, alpha_m=None, s_m=None) -> Dict[str, Tensor]:
    """dk_j = sum over the edges leaving j of s_e q_{tgt e};  dv_j = sum of alpha_e dz_{tgt e}.  Returns dk, dv, dk_m, dv_m."""
    q, dz, alpha, s = (t.to(dtype) for t in (q, dz, alpha, s))
    dz_m = dz.abs() if dz_m is None else dz_m.to(dtype)
    alpha_m = alpha.abs() if alpha_m is None else alpha_m.to(dtype)
    s_m = s.abs() if s_m is None else s_m.to(dtype)
    zero = torch.zeros_like(q)
    return dict(dk=zero.index_add(0, src, s[:, None] * q[tgt]), dv=zero.index_add(0, src, alpha[:, None] * dz[tgt]),
                dk_m=zero.index_add(0, src, s_m[:, None] * q[tgt].abs()), dv_m=zero.index_add(0, src, alpha_m[:, None] * dz_m[tgt]))  # fmt: skip


def rel_time(last_update, src, t, mean: float, std: float) -> Tensor:
    """(|last_update[src] - t| - mean) / std as torch evaluates it on an int64 tensor: float32, in EVERY evaluation (the kernel's bits)."""
    rel = (((last_update.long()[src] - t.long()).abs() - mean) / std).to(torch.float32)
    assert rel.dtype == torch.float32
    return rel


def edge_attr_backward(rel, tw, tb, d_attr, dtype=F64, d_attr_m=None):
    """rel [E] float32, tw / tb [T], d_attr [E, T]:  gs = -sin(rel tw + tb) d_attr;  part = [gs rel | gs]  ([E, 2T]).  Returns (part, part_m)."""
    rel, tw, tb, d_attr = (t.to(dtype) for t in (rel, tw, tb, d_attr))
    d_attr_m = d_attr.abs() if d_attr_m is None else d_attr_m.to(dtype)
    arg, arg_m = rel[:, None] * tw[None, :] + tb[None, :], rel.abs()[:, None] * tw.abs()[None, :] + tb.abs()[None, :]
    gs, gs_m = -torch.sin(arg) * d_attr, (torch.sin(arg).abs() + arg_m) * d_attr_m
    return torch.cat([gs * rel[:, None], gs], 1), torch.cat([gs_m * rel.abs()[:, None], gs_m], 1)


def antisym_grad(dA, dtype=F64, dA_m=None):
    """A = W - W^T - gamma I:  dW = dA - dA^T.  Returns (dW, dW_m)."""
    dA = dA.to(dtype)
    dA_m = dA.abs() if dA_m is None else dA_m.to(dtype)
    return dA - dA.t(), dA_m + dA_m.t()


# ---- the whole backward -------------------------------------------------------------------------------------------------------------------------
def forward_saved(p, node_x, last_update, edge_index, t, msg, num_iters=1, mean_delta_t=0.0, std_delta_t=1.0, epsilon=0.1, gamma=0.1, dtype=F64):
    """What the saving forward keeps, in ``dtype``: x at the entry of every iteration, out, edge_attr, eproj, the clamped edge list, rel."""
    c = lambda v: v.detach().to(dtype)
    U = node_x.shape[0]
    src, tgt = edge_index[0].long().clamp(0, max(U - 1, 0)), edge_index[1].long().clamp(0, max(U - 1, 0))
    rel = rel_time(last_update, src, t, mean_delta_t, std_delta_t)
    tw, tb = c(p['time_enc.lin.weight'])[:, 0], c(p['time_enc.lin.bias'])
    edge_attr = torch.cat([c(msg), torch.cos(c(rel)[:, None] * tw[None, :] + tb[None, :])], -1)
    ep = edge_attr @ c(p['aconv.phi.lin_edge.weight']).T
    x = c(node_x) @ c(p['enc_x.weight']).T + c(p['enc_x.bias'])
    M = x.shape[1]
    W = c(p['aconv.W'])
    A = W - W.T - gamma * torch.eye(M, dtype=dtype)
    W4 = [c(p[f'aconv.phi.lin_{n}.weight']) for n in ('query', 'key', 'value')] + [A]
    b4 = [c(p[f'aconv.phi.lin_{n}.bias']) for n in ('query', 'key', 'value')] + [c(p['aconv.bias'])]
    xs = []
    scale = 1.0 / math.sqrt(M)
    for _ in range(num_iters):
        xs.append(x)
        q, k, v, h = (x @ Wb.T + bb for Wb, bb in zip(W4, b4))
        if ep.shape[0]:
            alpha = _segment_softmax((q[tgt] * (k[src] + ep)).sum(-1) * scale, tgt, U)
            h = h + torch.zeros_like(x).index_add(0, tgt, alpha[:, None] * (v[src] + ep))
        x = x + epsilon * torch.tanh(h)
    if not xs:
        xs.append(x)
    return dict(xs=xs, x_last=x, out=torch.tanh(x), edge_attr=edge_attr, ep=ep, src=src, tgt=tgt, rel=rel, W4=W4, b4=b4, tw=tw, tb=tb, node_x=c(node_x),
                Wx=c(p['enc_x.weight']), We=c(p['aconv.phi.lin_edge.weight']), num_iters=num_iters, epsilon=epsilon, scale=scale, D=msg.shape[1])


def backward(sv, g, dtype=F64) -> Dict[str, tuple]:
    """The launch list of ``tgmx_ctan_backward`` as formulas: name -> (gradient, magnitude) for every parameter and for ``node_x``."""
    g = g.to(dtype)
    out, U, M = sv['out'].to(dtype), sv['out'].shape[0], sv['out'].shape[1]
    W4, src, tgt, ep, E = [w.to(dtype) for w in sv['W4']], sv['src'], sv['tgt'], sv['ep'].to(dtype), sv['ep'].shape[0]
    gx, gx_m = g * (1 - out * out), g.abs() * (1 + out * out)
    dW4, dW4_m = [torch.zeros(M, M, dtype=dtype) for _ in range(4)], [torch.zeros(M, M, dtype=dtype) for _ in range(4)]
    db4, db4_m = [torch.zeros(M, dtype=dtype) for _ in range(4)], [torch.zeros(M, dtype=dtype) for _ in range(4)]
    de, de_m = torch.zeros_like(ep), torch.zeros_like(ep)
    for it in range(sv['num_iters'] - 1, -1, -1):
        x = sv['xs'][it].to(dtype)
        q, k, v, h4 = (x @ Wb.T + bb.to(dtype) for Wb, bb in zip(W4, sv['b4']))
        tp = target_pass(q, k, v, h4, ep, src, tgt, gx, sv['scale'], sv['epsilon'], dtype, gx_m=gx_m)
        sp = source_pass(q, tp['dz'], src, tgt, tp['alpha'], tp['s'], dtype, dz_m=tp['dz_m'], alpha_m=tp['alpha_m'], s_m=tp['s_m'])
        de, de_m = de + tp['de'], de_m + tp['de_m']
        d4, d4_m = [tp['dq'], sp['dk'], sp['dv'], tp['dz']], [tp['dq_m'], sp['dk_m'], sp['dv_m'], tp['dz_m']]
        for b in range(4):
            dW4[b], dW4_m[b] = dW4[b] + d4[b].T @ x, dW4_m[b] + d4_m[b].T @ x.abs()
            db4[b], db4_m[b] = db4[b] + d4[b].sum(0), db4_m[b] + d4_m[b].sum(0)
            gx, gx_m = gx + d4[b] @ W4[b], gx_m + d4_m[b] @ W4[b].abs()
    res = {}
    for b, n in enumerate(('query', 'key', 'value')):
        res[f'aconv.phi.lin_{n}.weight'], res[f'aconv.phi.lin_{n}.bias'] = (dW4[b], dW4_m[b]), (db4[b], db4_m[b])
    res['aconv.bias'] = (db4[3], db4_m[3])
    res['aconv.W'] = antisym_grad(dW4[3], dtype, dW4_m[3])
    nx, Wx, We, D = sv['node_x'].to(dtype), sv['Wx'].to(dtype), sv['We'].to(dtype), sv['D']
    res['enc_x.weight'], res['enc_x.bias'] = (gx.T @ nx, gx_m.T @ nx.abs()), (gx.sum(0), gx_m.sum(0))
    res['node_x'] = (gx @ Wx, gx_m @ Wx.abs())
    ea = sv['edge_attr'].to(dtype)
    res['aconv.phi.lin_edge.weight'] = (de.T @ ea, de_m.T @ ea.abs())
    part, part_m = edge_attr_backward(sv['rel'], sv['tw'], sv['tb'], de @ We[:, D:], dtype, d_attr_m=de_m @ We[:, D:].abs())
    T = sv['tw'].shape[0]
    res['time_enc.lin.weight'] = (part[:, :T].sum(0)[:, None], part_m[:, :T].sum(0)[:, None])
    res['time_enc.lin.bias'] = (part[:, T:].sum(0), part_m[:, T:].sum(0))
    assert E == src.numel()
    return res


# ---- cases of the kernels alone -----------------------------------------------------------------------------------------------------------------
def kernel_case(C: int, U: int = 40, seed: int = 0, lens=SEG_LENS):
    """Targets 0, 1, ... with ``lens`` incoming edges (the rest none), in shuffled edge order; sources drawn so that node i also has
    ``lens[i]`` OUTGOING edges (a second shuffle of the same multiset).  randn rows, scaled so that scores stay O(1)."""
    g = torch.Generator().manual_seed(seed * 7919 + C)
    ids = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    E = ids.numel()
    tgt, src = ids[torch.randperm(E, generator=g)], ids[torch.randperm(E, generator=g)]
    q, k, v, h4, gx = (torch.randn(U, C, generator=g) for _ in range(5))
    ep = torch.randn(E, C, generator=g)
    return dict(U=U, C=C, E=E, src=src, tgt=tgt, q=q, k=k, v=v, h4=h4, gx=gx, ep=ep, scale=1.0 / math.sqrt(C), eps=0.5,
                de_old=torch.randn(E, C, generator=g), in_deg=torch.bincount(tgt, minlength=U), out_deg=torch.bincount(src, minlength=U))


def grouped(key: Tensor, U: int):
    """(order, lo, hi): ids stably sorted by key and every key's range -- what tgmx_segment_sort gives."""
    order = torch.argsort(key, stable=True)
    sk = key[order]
    r = torch.arange(U)
    return order, torch.searchsorted(sk, r), torch.searchsorted(sk, r, right=True)


def parse_mode(value: Optional[str]) -> str:
    """``TGMX_CTAN_BWD`` as the product reads it: 'py' and 'torch' are themselves, anything else is the one call."""
    return value if value in ('py', 'torch') else 'native'
