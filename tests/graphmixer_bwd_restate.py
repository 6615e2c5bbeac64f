"""The backward of GraphMixer's encoder and of one MLP-Mixer block restated in float64, pure torch on the CPU, in the manner of
``ctan_bwd_restate.py``: written out from the formulas with explicit masks (the valid slots of the link mean, the four dropout sites of a
layer), no autograd.  Every block returns values and, under the same names with ``_m``, the same formula with every term replaced by its
absolute value.  A worst-case rounding bound for a float32 evaluation is ``chain * 2^-24 * magnitude`` with ``chain`` from the helpers
below (counted from ``csrc/mixer_bwd.hip``).

Magnitudes follow ``gclstm_bwd_restate``'s rules: a difference counts as the sum of its terms' magnitudes (``x - mean`` as ``|x| + mean|x|``);
a function of a rounded value counts as its own value plus its derivative times the argument's magnitude (``rstd`` as ``rstd + rstd^3
mag(var) / 2``; ``gelu(a)`` as ``mag(gelu)(a) + mag(gelu')(a) mag(a)`` and ``gelu'(a)`` with ``gelu''(a) = phi(a) (2 - a^2)``, where GELU's own
magnitude is ``|a| (1 + |erf|) / 2``: the kernels form ``1 + erf(a / sqrt 2)`` as a sum, like the forward and like torch, and for negative
``a`` that sum cancels).

The forward with masks (:func:`mixer_forward`, :func:`encoder_forward`) is plain torch, so float64 autograd can differentiate it: the
backward formulas are pinned to that in ``tests/test_graphmixer_train_cpu.py``, and with unit masks the forward is
``graphmixer_restate``'s.  Dropout masks: ``oracle.dropout_ref.dropout_scale`` with stream ``first + 4 l + site`` and the element index the
flat index in the site's tensor -- 0 token hidden [S, C, Ht], 1 token output [S, C, K], 2 channel hidden [S K, Hc], 3 channel output
[S K, C].  Nothing here imports the product.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
from torch import Tensor

from oracle.dropout_ref import dropout_scale
from oracle.tgat_bwd_ref import EPS, F64  # noqa: F401  (EPS: re-exported for the tests)
from oracle.tgn_bwd_ref import TRANSCENDENTAL_OPS

PAD = -1
LAYER_NAMES = ('token_norm.weight', 'token_norm.bias', 'token_feedforward.ffn.0.weight', 'token_feedforward.ffn.0.bias',
               'token_feedforward.ffn.3.weight', 'token_feedforward.ffn.3.bias', 'channel_norm.weight', 'channel_norm.bias',
               'channel_feedforward.ffn.0.weight', 'channel_feedforward.ffn.0.bias', 'channel_feedforward.ffn.3.weight',
               'channel_feedforward.ffn.3.bias')  # fmt: skip


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------
def token_chain(K: int, Ht: int) -> int:
    """float32 operations on the longest chain into an element of dx, plus 8, counted from mixer_token_backward_kernel: the mean and the
    variance (K each, 2 for the divisions), rstd (3), x-hat and xn (4), the mask (1), a pre-activation (K + 1), its GELU and GELU' (erff and
    expf, 6 products and sums), dh (K), da (2), dxn (Ht), the two means (2 K + 2), dx (6)."""
    return 2 * K + 2 + 3 + 4 + 1 + K + 1 + 2 * TRANSCENDENTAL_OPS + 6 + K + 2 + Ht + 2 * K + 2 + 6 + 8


def gelu_chain() -> int:
    """erff and expf, the scaled argument (1), Phi (2), a phi (3), their sum (1), the mask and dh (2), plus 8"""
    return 2 * TRANSCENDENTAL_OPS + 1 + 2 + 3 + 1 + 2 + 8


def tail_chain() -> int:
    """one division, plus 8"""
    return 1 + 8


# ---- pieces -----------------------------------------------------------------------------------------------------------------------------------
def gelu(a: Tensor) -> Tensor:
    return 0.5 * a * (1 + torch.erf(a / math.sqrt(2.0)))


def _phi(a: Tensor) -> Tensor:
    return torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def gelu_grad(a: Tensor) -> Tensor:
    """Phi(a) + a phi(a)"""
    return 0.5 * (1 + torch.erf(a / math.sqrt(2.0))) + a * _phi(a)


def gelu_m(a: Tensor) -> Tensor:
    """|a| (1 + |erf|) / 2: the kernels form 1 + erf(a / sqrt 2) as a sum (as the forward's GELU does), which cancels for negative a"""
    return 0.5 * a.abs() * (1 + torch.erf(a / math.sqrt(2.0)).abs())


def gelu_grad_m(a: Tensor) -> Tensor:
    """(1 + |erf|) / 2 + |a| phi(a): the same for gelu'"""
    return 0.5 * (1 + torch.erf(a / math.sqrt(2.0)).abs()) + a.abs() * _phi(a)


def gelu_grad2(a: Tensor) -> Tensor:
    return _phi(a) * (2 - a * a)


def layer_masks(p: float, seed: int, first_stream: int, layer: int, S: int, K: int, C: int, Ht: int, Hc: int, dtype=F64) -> List[Tensor]:
    """[m0 [S, C, Ht], m1 [S, C, K], m2 [S K, Hc], m3 [S K, C]]: the scales 1 / (1 - p) or 0 of a layer's four sites (all ones at p = 0)."""
    shapes = ((S, C, Ht), (S, C, K), (S * K, Hc), (S * K, C))
    return [(dropout_scale(p, seed, first_stream + 4 * layer + s, sh) if min(sh) else torch.ones(sh)).to(dtype) for s, sh in enumerate(shapes)]


def unit_masks(S: int, K: int, C: int, Ht: int, Hc: int, dtype=F64) -> List[Tensor]:
    return layer_masks(0.0, 0, 0, 0, S, K, C, Ht, Hc, dtype)


def _layer(sd: Dict[str, Tensor], prefix: str, dtype) -> List[Tensor]:
    return [sd[prefix + n].to(dtype) for n in LAYER_NAMES]


def _norm(x: Tensor, x_m: Tensor, eps: float):
    """LayerNorm over the last dimension without its affine part: (x-hat, rstd) and their magnitudes."""
    mean, mean_m = x.mean(-1, keepdim=True), x_m.mean(-1, keepdim=True)
    d, d_m = x - mean, x_m + mean_m
    var, var_m = (d * d).mean(-1, keepdim=True), (d_m * d_m).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    rstd_m = rstd + 0.5 * rstd**3 * var_m
    return d * rstd, d_m * rstd_m, rstd, rstd_m


def _norm_backward(gk, gk_m, xh, xh_m, rstd, rstd_m):
    """rstd (g - mean(g) - x-hat mean(g x-hat)) over the last dimension, g = the gradient at x-hat."""
    a1, a1_m = gk.mean(-1, keepdim=True), gk_m.mean(-1, keepdim=True)
    a2, a2_m = (gk * xh).mean(-1, keepdim=True), (gk_m * xh_m).mean(-1, keepdim=True)
    return rstd * (gk - a1 - xh * a2), rstd_m * (gk_m + a1_m + xh_m * a2_m)


# ---- the token block ------------------------------------------------------------------------------------------------------------------------------
def token_backward(P: List[Tensor], x: Tensor, dz1: Tensor, m0: Tensor, m1: Tensor, eps: float = 1e-5, dz1_m: Optional[Tensor] = None,
                   x_m: Optional[Tensor] = None) -> Dict[str, Tensor]:  # fmt: skip
    """x, dz1 [S, K, C]; P = the layer's parameters (``LAYER_NAMES`` order).  z1 = x + m1 (W2 (m0 gelu(W1 LN_K(x) + b1)) + b2) per column:

        do = dz1 m1;  dW2 = do^T hd;  db2 = sum do;  dh = do W2;  da = dh m0 gelu'(a);  dW1 = da^T xn;  db1 = sum da;  dxn = da W1
        d tok_b = sum dxn;  d tok_g = sum dxn x-hat;  dx = rstd (g dxn - mean(g dxn) - x-hat mean(g dxn x-hat)) + dz1

    Returns dx [S, K, C], the six parameter gradients under their ``LAYER_NAMES`` names, the kernel's rows (``rows``: [S C, 4 K + 2 Ht] =
    do | xn | dxn | dxn x-hat | hd | da) and the magnitudes of all of them (``*_m``)."""
    tg, tb, W1, b1, W2, _ = P[:6]
    S, K, C = x.shape
    xt, d = x.transpose(1, 2), dz1.transpose(1, 2)  # [S, C, K]
    xt_m = xt.abs() if x_m is None else x_m.transpose(1, 2)
    d_m = d.abs() if dz1_m is None else dz1_m.transpose(1, 2)
    xh, xh_m, rstd, rstd_m = _norm(xt, xt_m, eps)
    xn, xn_m = xh * tg + tb, xh_m * tg.abs() + tb.abs()
    a, a_m = xn @ W1.T + b1, xn_m @ W1.abs().T + b1.abs()
    ge = gelu(a)
    hd, hd_m = ge * m0, (gelu_m(a) + gelu_grad_m(a) * a_m) * m0
    do, do_m = d * m1, d_m * m1
    dh, dh_m = do @ W2, do_m @ W2.abs()
    gp, gp_m = gelu_grad(a), gelu_grad_m(a) + gelu_grad2(a).abs() * a_m
    da, da_m = dh * m0 * gp, dh_m * m0 * gp_m
    dxn, dxn_m = da @ W1, da_m @ W1.abs()
    gxh, gxh_m = dxn * xh, dxn_m * xh_m
    du, du_m = _norm_backward(dxn * tg, dxn_m * tg.abs(), xh, xh_m, rstd, rstd_m)
    flat = lambda t: t.reshape(S * C, -1)
    both = lambda A, B: torch.einsum('scm,scn->mn', A, B)
    res = dict(dx=(du + d).transpose(1, 2), dx_m=(du_m + d_m).transpose(1, 2),
               rows=torch.cat([flat(t) for t in (do, xn, dxn, gxh, hd, da)], 1), rows_m=torch.cat([flat(t) for t in (do_m, xn_m, dxn_m, gxh_m, hd_m, da_m)], 1))  # fmt: skip
    for name, v, m in zip(LAYER_NAMES[:6], (gxh.sum((0, 1)), dxn.sum((0, 1)), both(da, xn), da.sum((0, 1)), both(do, hd), do.sum((0, 1))),
                          (gxh_m.sum((0, 1)), dxn_m.sum((0, 1)), both(da_m, xn_m), da_m.sum((0, 1)), both(do_m, hd_m), do_m.sum((0, 1)))):  # fmt: skip
        res[name], res[name + '_m'] = v, m
    return res


# ---- the channel FFN ------------------------------------------------------------------------------------------------------------------------------
def channel_backward(P: List[Tensor], z1: Tensor, gz: Tensor, m2: Tensor, m3: Tensor, eps: float = 1e-5, gz_m: Optional[Tensor] = None,
                     z1_m: Optional[Tensor] = None) -> Dict[str, Tensor]:  # fmt: skip
    """z1, gz [R, C].  z = z1 + m3 (W2 (m2 gelu(W1 y + b1)) + b2), y = LN_C(z1):

        gt = gz m3;  dW2 = gt^T hd;  db2 = sum gt;  dh = gt W2;  da = dh m2 gelu'(a);  dW1 = da^T y;  db1 = sum da;  dy = da W1
        d ch_b = sum dy;  d ch_g = sum dy x-hat;  dz1 = gz + rstd (g dy - mean(g dy) - x-hat mean(g dy x-hat))

    Returns dz1 and the six parameter gradients under their ``LAYER_NAMES`` names, with magnitudes."""
    cg, cb, W1, b1, W2, _ = P[6:]
    gz_m = gz.abs() if gz_m is None else gz_m
    z1_m = z1.abs() if z1_m is None else z1_m
    xh, xh_m, rstd, rstd_m = _norm(z1, z1_m, eps)
    y, y_m = xh * cg + cb, xh_m * cg.abs() + cb.abs()
    a, a_m = y @ W1.T + b1, y_m @ W1.abs().T + b1.abs()
    ge = gelu(a)
    hd, hd_m = ge * m2, (gelu_m(a) + gelu_grad_m(a) * a_m) * m2
    gt, gt_m = gz * m3, gz_m * m3
    dh, dh_m = gt @ W2, gt_m @ W2.abs()
    da, da_m = dh * m2 * gelu_grad(a), dh_m * m2 * (gelu_grad_m(a) + gelu_grad2(a).abs() * a_m)
    dy, dy_m = da @ W1, da_m @ W1.abs()
    du, du_m = _norm_backward(dy * cg, dy_m * cg.abs(), xh, xh_m, rstd, rstd_m)
    res = dict(dz1=gz + du, dz1_m=gz_m + du_m)
    for name, v, m in zip(LAYER_NAMES[6:], ((dy * xh).sum(0), dy.sum(0), da.T @ y, da.sum(0), gt.T @ hd, gt.sum(0)),
                          ((dy_m * xh_m).sum(0), dy_m.sum(0), da_m.T @ y_m, da_m.sum(0), gt_m.T @ hd_m, gt_m.sum(0))):  # fmt: skip
        res[name], res[name + '_m'] = v, m
    return res


# ---- one block and the encoder, forward (plain torch: autograd can differentiate it) and backward (formulas) -----------------------------------------
def mixer_forward(P: List[Tensor], x: Tensor, masks: List[Tensor], eps: float = 1e-5, keep: Optional[dict] = None) -> Tensor:
    """One MLP-Mixer block on x [S, K, C] with the four sites' scales; ``keep`` receives z1 (the token block's output)."""
    tg, tb, W1, b1, W2, b2, cg, cb, V1, c1, V2, c2 = P
    S, K, C = x.shape
    m0, m1, m2, m3 = masks
    xt = x.transpose(1, 2)
    xh = (xt - xt.mean(-1, keepdim=True)) * (xt.var(-1, unbiased=False, keepdim=True) + eps) ** -0.5
    o = ((gelu((xh * tg + tb) @ W1.T + b1) * m0) @ W2.T + b2) * m1
    z1 = x + o.transpose(1, 2)
    if keep is not None:
        keep['z1'] = z1.detach()
    zh = (z1 - z1.mean(-1, keepdim=True)) * (z1.var(-1, unbiased=False, keepdim=True) + eps) ** -0.5
    h = gelu((zh * cg + cb) @ V1.T + c1) * m2.view(S, K, -1)
    return z1 + (h @ V2.T + c2) * m3.view(S, K, C)


def mixer_backward(P: List[Tensor], x: Tensor, z1: Tensor, g: Tensor, masks: List[Tensor], eps: float = 1e-5, g_m: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """The block's backward from the saved x and z1: dx and the twelve parameter gradients (``LAYER_NAMES``), with magnitudes."""
    S, K, C = x.shape
    m0, m1, m2, m3 = masks
    ch = channel_backward(P, z1.reshape(S * K, C), g.reshape(S * K, C), m2, m3, eps, gz_m=None if g_m is None else g_m.reshape(S * K, C))
    tk = token_backward(P, x, ch['dz1'].view(S, K, C), m0, m1, eps, dz1_m=ch['dz1_m'].view(S, K, C))
    res = {k: v for k, v in ch.items() if not k.startswith('dz1')}
    res.update({k: v for k, v in tk.items() if not k.startswith('rows')})
    return res


def time_features(sd, seed_times, nbr_edge_time, dtype=F64) -> Tensor:
    dt = (seed_times[:, None].long() - nbr_edge_time.long()).to(torch.float32).to(dtype).unsqueeze(-1)
    return torch.cos(dt * sd['time_encoder.w.weight'].to(dtype).view(-1) + sd['time_encoder.w.bias'].to(dtype))


def encoder_forward(sd: Dict[str, Tensor], num_layers: int, nbr_edge_x, seed_times, nbr_edge_time, nbr_nids, seeds, tg_lists, node_feat,
                    masks: Optional[List[List[Tensor]]] = None, dtype=F64, keep: Optional[dict] = None) -> Tensor:  # fmt: skip
    """``graphmixer_restate.encoder_forward`` with a layer's four dropout scales (``masks[l]``; None: all ones); ``keep`` receives what
    the saving forward keeps: x0, per layer z and z1, cat."""
    g = lambda n: sd[n].to(dtype)
    S, K, D = nbr_edge_x.shape
    x0 = torch.cat([nbr_edge_x.to(dtype), time_features(sd, seed_times, nbr_edge_time, dtype)], -1)
    z = x0 @ g('projection_layer.weight').T + g('projection_layer.bias')
    zs, z1s = [], []
    for l in range(num_layers):
        P = _layer(sd, f'mlp_mixers.{l}.', dtype)
        m = masks[l] if masks is not None else unit_masks(S, K, D, P[2].shape[0], P[8].shape[0], dtype)
        k = {}
        zs.append(z.detach())
        z = mixer_forward(P, z, m, keep=k)
        z1s.append(k['z1'])
    valid = (nbr_nids != PAD).to(dtype)
    z_link = (z * valid.unsqueeze(-1)).sum(1) / valid.sum(1, keepdim=True).clamp(min=1)
    x = node_feat.to(dtype)
    tg = torch.zeros((S, x.shape[1]), dtype=dtype)
    for i, lst in enumerate(tg_lists):
        if lst:
            tg[i] = x[torch.tensor(lst, dtype=torch.long)].mean(0)
    cat = torch.cat([z_link, tg + x[seeds.long()]], 1)
    if keep is not None:
        keep.update(x0=x0.detach(), zs=zs, z1s=z1s, cat=cat.detach(), valid=valid)
    return cat @ g('output_layer.weight').T + g('output_layer.bias')


def encoder_backward(sd: Dict[str, Tensor], num_layers: int, kept: dict, g: Tensor, masks: Optional[List[List[Tensor]]] = None, dtype=F64) -> Dict[str, tuple]:
    """The launch list of ``tgmx_graphmixer_backward`` as formulas: parameter name -> (gradient, magnitude)."""
    g = g.to(dtype)
    g_m = g.abs()
    x0, cat, valid = kept['x0'], kept['cat'], kept['valid']
    S, K = valid.shape
    D = x0.shape[-1] - sd['time_encoder.w.bias'].numel()
    Wo = sd['output_layer.weight'].to(dtype)
    res = {'output_layer.weight': (g.T @ cat, g_m.T @ cat.abs()), 'output_layer.bias': (g.sum(0), g_m.sum(0))}
    dcat, dcat_m = g @ Wo[:, :D], g_m @ Wo[:, :D].abs()
    w = (valid / valid.sum(1, keepdim=True).clamp(min=1)).unsqueeze(-1)  # 1 / max(1, valid_s) on the valid slots, 0 on the pads
    gz, gz_m = w * dcat[:, None, :], w * dcat_m[:, None, :]
    for l in range(num_layers - 1, -1, -1):
        P = _layer(sd, f'mlp_mixers.{l}.', dtype)
        m = masks[l] if masks is not None else unit_masks(S, K, D, P[2].shape[0], P[8].shape[0], dtype)
        r = mixer_backward(P, kept['zs'][l], kept['z1s'][l], gz, m, g_m=gz_m)
        for n in LAYER_NAMES:
            res[f'mlp_mixers.{l}.{n}'] = (r[n], r[n + '_m'])
        gz, gz_m = r['dx'], r['dx_m']
    f, f_m = gz.reshape(S * K, D), gz_m.reshape(S * K, D)
    x0f = x0.reshape(S * K, -1)
    res['projection_layer.weight'], res['projection_layer.bias'] = (f.T @ x0f, f_m.T @ x0f.abs()), (f.sum(0), f_m.sum(0))
    return res


def tail_backward(dcat: Tensor, nids: Tensor, K: int, dtype=F64) -> Tensor:
    """dz [S K, C] = nids != -1 ? dcat[s] / max(1, valid_s) : 0."""
    valid = (nids != PAD).to(dtype)
    w = valid / valid.sum(1, keepdim=True).clamp(min=1)
    return (w.unsqueeze(-1) * dcat.to(dtype)[:, None, :]).reshape(nids.shape[0] * K, -1)


def parse_mode(value: Optional[str], default: str = 'native') -> str:
    """``TGMX_GRAPHMIXER_BWD`` as the product reads it: 'native', 'py' and 'torch' are themselves, anything else is the default."""
    return value if value in ('native', 'py', 'torch') else default
