"""Training path of ``TPNet`` (tgm/nn/encoder/tpnet.py under ``loss.backward()``): a ``torch.autograd.Function`` whose forward is the
inference call in its saving form (``tgmx_tpnet_forward_train``: the same kernels in the same order, so with dropout off the grad-enabled
forward returns the bits of the no-grad one) and whose backward is ONE native call (``tgmx_tpnet_backward``, ``csrc/tpnet_bwd.hip``), with
g = [dz_src; dz_dst] [2B, E]:

    the token mean                -> ``tgmx_tpnet_mean_backward``: gz[q k + j] = g[q] / k on every slot (TPNet's mean is not masked)
    per layer, last first:
      the channel block           -> the launches of ``tgmx_graphmixer_backward``'s channel block (``_graphmixer_train._LayerRun.channel``)
      the token block             -> ``tgmx_tpnet_token_backward`` (the forward's refined column mean): gz <- dx, and ONE row of partial sums
                                     per sequence; one ``tgmx_colsum`` over the 2B rows gives the six token-block gradients
    the projection                -> d W2 = gz^T hp, d b2, dhp = gz W2 masked by hp > 0, d W0 = dhp^T x0, d b0; of dx0 only the time columns
                                     and the two pair blocks are formed (GEMMs against packed transposed slices of W0)
    the time encoder              -> ``tgmx_tpnet_time_backward`` rows, two ``tgmx_colsum``
    the pair-feature MLP          -> d W2, d b2, dfh = dpf W2 masked by feat_h > 0, d W1, d b1 over the 2R rows

No gradient goes to ``node_x``, the edge features or the tables: a call that asks for one is outside the envelope and keeps the composed
path, as does ``TGMX_TPNET_BWD=torch``.  ``TGMX_TPNET_BWD=py`` issues the backward's launches one ctypes call each from
:func:`backward_per_launch` -- the readable specification, the same bits.  Every sum has a fixed order (no float atomics): two runs give the
same bits.

What is saved: the KEEPING form for the two ReLU hiddens.  Kept per call, in buffers the call owns: ``feat`` [2R, ldf] (the pair-feature
MLP's input), ``feat_h`` [2R, ldfh], ``x0`` [R, ldx0], ``hp`` [R, ldhp], per layer the token block's input ``z`` and output ``z1``, and one
double per token row (``lg`` = log(gap + 1), -1 on a pad slot).  The backward reads NONE of the caller's tensors: the sampler's outputs are
pooled and rewritten by the next batch.  LayerNorm outputs and the channel FFN's pre-activations are recomputed.  At the example shape
(B 200, k 32: R = 12 800; W = 472, od = 36, E = 172, 2 layers) that is 3.7 MB of feat, 14.7 MB of feat_h, 24.2 MB of x0, 17.6 MB of hp,
35.2 MB of z | z1 and 0.1 MB of lg: 95.5 MB a call (recomputing feat_h and hp instead would keep 63.2 MB and add two GEMMs).

The weights the backward reads -- and the transposes and column slices it multiplies by -- are copied once per parameter version by
``tgmx_pack2d`` (:func:`backward_weights`) and bound to the call at FORWARD time: forward A, optimizer step, forward B, backward B,
backward A differentiates A with A's weights.

Dropout (train mode, p > 0): the four sites per layer and the element indexing of ``tgmx_graphmixer_forward_train`` over Q = 2B sequences,
seed ``torch.initial_seed()``, stream ``call * 64 + 4 l + site``, regenerated in the backward, never stored.
"""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace
from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _native
from ._fwd_plumbing import check_supported, up4
from ._gclstm_train import _grad_views, _rows
from ._graphmixer_train import _LAYER_FIELDS, _LayerRun, _layer_params, next_drop
from ._paramver import param_key, param_list

DEFAULT = 'native'  # chosen by tools/bench_tpnet_train.py against the composed path
_CH_FIELDS = _LAYER_FIELDS[6:]
_HEAD_FIELDS = ('d_tw', 'd_tb', 'd_proj_w0', 'd_proj_b0', 'd_proj_w2', 'd_proj_b2', 'd_rp_w1', 'd_rp_b1', 'd_rp_w2', 'd_rp_b2')


def mode() -> str:
    """'native', 'py' or 'torch': ``TGMX_TPNET_BWD``, anything else is the default."""
    m = os.environ.get('TGMX_TPNET_BWD', '')
    return m if m in ('native', 'py', 'torch') else DEFAULT


def train_supported(K: int, C: int, Ht: int) -> bool:
    """A sequence's tile fits both token kernels (``tgmx_tpnet_train_supported``: the one function the forward and the backward go by)."""
    return bool(_native.load().tgmx_tpnet_train_supported(int(K), int(C), int(Ht)))


def part_floats(K: int, Ht: int) -> int:
    """Length of ``tgmx_tpnet_token_backward``'s partial row: [do^T hd | da^T xn | sum do | sum dxn | sum dxn xhat | sum da]."""
    return 2 * K * Ht + 3 * K + Ht


def _head_params(module) -> list:
    """The parameters outside the mixers in ``_HEAD_FIELDS``' order (None where the module has no pair features)."""
    tw, pl, rp = module.time_encoder.w, module.projection_layer, module.random_projections
    rpp = [None] * 4 if rp is None else [rp.mlp[0].weight, rp.mlp[0].bias, rp.mlp[2].weight, rp.mlp[2].bias]
    return [tw.weight, tw.bias, pl[0].weight, pl[0].bias, pl[2].weight, pl[2].bias] + rpp


def in_envelope(module, a: dict) -> bool:
    """The native training path takes this call (the conditions of the issue / README): gradients on with a parameter that wants one, no
    autocast, not ``torch`` mode, float32 contiguous parameters on one device, inputs that want no gradient, a ``Time2Vec`` encoder, at most
    4 tables, one eps and one dropout p, mixers the native kernels take, at most 8 layers, B > 0."""
    node_x, nbr_x = a['node_x'], a['nbr_x']
    dev = node_x.device
    if mode() == 'torch' or a['B'] <= 0 or not torch.is_grad_enabled() or torch.is_autocast_enabled(dev.type):
        return False
    if node_x.requires_grad or nbr_x.requires_grad:
        return False
    if not hasattr(module.time_encoder, 'w') or module.num_layers > _native.MIXER_MAX_LAYERS:
        return False
    rp = module.random_projections
    if rp is not None and rp.num_layer + 1 > _native.TPNET_PAIR_MAX_LEVELS:
        return False
    weights = [p for p in _head_params(module) if p is not None] + [p for m in module.mlp_mixers for p in _layer_params(m)]
    if any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in weights):
        return False
    if not any(p.requires_grad for p in weights):
        return False
    p = float(module.dropout)
    eps = set()
    for m in module.mlp_mixers:
        try:
            m._check_native()
        except NotImplementedError:
            return False
        tf, cf = m.token_feedforward.ffn, m.channel_feedforward.ffn
        if any(float(d.p) != p for d in (tf[2], tf[4], cf[2], cf[4])) or cf[0].out_features < 1:
            return False
        if m.num_tokens != module.num_neighbors or m.num_channels != module.output_dim:
            return False
        if not train_supported(m.num_tokens, m.num_channels, tf[0].out_features):
            return False
        eps |= {float(m.token_norm.eps), float(m.channel_norm.eps)}
    return 0.0 <= p < 1.0 and len(eps) <= 1


# ---- the weights of a call -------------------------------------------------------------------------------------------------------------------
def backward_weights(module) -> SimpleNamespace:
    """What the backward reads of the parameters, copied by ``tgmx_pack2d`` and cached on ``module`` against their versions: per mixer the
    ``tgmx_mixer_layer_t`` fields it needs, ``ch_w1T`` [E, Hc] and ``ch_w2T`` [Hc, E]; ``tw`` / ``tb``; ``proj_w2T`` [2E, E]; the transposed
    column slices of ``projection_layer.0.weight`` somebody reads: ``w0T_time`` [dT, 2E], ``w0T_pair0`` / ``w0T_pair1`` [od, 2E];
    ``rp_w2T`` [4 od, od].  A call keeps the object it got at forward time."""
    d = module.__dict__
    key = param_key(module)
    if d.get('_tgmx_tp_wkey') == key:
        return d['_tgmx_tp_w']
    dev = module.projection_layer[0].weight.device
    heads = _head_params(module)
    dN, dT, dE = module.node_feat_dim, module.time_feat_dim, module.edge_x_dim
    od = 0 if module.random_projections is None else module.random_projections.out_dim
    base = dN + dT + dE
    w0 = heads[2].detach()
    plan = [('tw', -1, heads[0].detach().reshape(1, -1), False), ('tb', -1, heads[1].detach(), False), ('proj_w2T', -1, heads[4].detach(), True)]  # (name, layer, source, transpose)
    if dT:
        plan.append(('w0T_time', -1, w0[:, dN : dN + dT], True))
    if od:
        plan += [('w0T_pair0', -1, w0[:, base : base + od], True), ('w0T_pair1', -1, w0[:, base + od : base + 2 * od], True), ('rp_w2T', -1, heads[8].detach(), True)]
    for l, m in enumerate(module.mlp_mixers):
        ps = _layer_params(m)
        for name, p in zip(_LAYER_FIELDS, ps):
            if name not in ('tok_b2', 'ch_w2', 'ch_b2'):  # (the backward reads neither the second Linears' biases nor W2 itself)
                plan.append((name, l, p.detach(), False))
        plan += [('ch_w1T', l, ps[8].detach(), True), ('ch_w2T', l, ps[10].detach(), True)]
    views = _grad_views([tuple(t.shape) if not tr else (t.shape[1], t.shape[0]) for _, _, t, tr in plan], dev)
    jobs = []
    for (name, l, t, tr), v in zip(plan, views):
        if t.numel() == 0:
            continue
        src = t if t.dim() == 2 else t.view(1, -1)
        rows, cols = (src.shape[1], src.shape[0]) if tr else tuple(src.shape)  # the extent in dst coordinates
        j = _native.PackJob()
        j.src, j.dst, j.src_ld, j.dst_ld, j.rows, j.cols, j.dst_rows, j.dst_cols, j.transpose = src.data_ptr(), v.data_ptr(), src.stride(0), cols, rows, cols, rows, cols, int(tr)
        jobs.append(j)
    lib, st = _native.load(), _native.stream_ptr()
    for i in range(0, len(jobs), 32):  # TGMX_PACK_MAX_JOBS
        chunk = (_native.PackJob * len(jobs[i : i + 32]))(*jobs[i : i + 32])
        _native.check(lib.tgmx_pack2d(chunk, len(chunk), st), 'tgmx_pack2d')
    w = SimpleNamespace(layers=[dict() for _ in module.mlp_mixers], head={}, views=views,
                        hidden=[(m.token_feedforward.ffn[0].out_features, m.channel_feedforward.ffn[0].out_features) for m in module.mlp_mixers])
    for (name, l, t, tr), v in zip(plan, views):
        if l < 0:
            w.head[name] = v
        else:
            w.layers[l][name] = v
    d['_tgmx_tp_w'], d['_tgmx_tp_wkey'] = w, key
    return w


def _fill_weights(t, w: SimpleNamespace) -> None:
    """The weight pointers of ``tgmx_tpnet_bwd_t`` from the call's packed copies (empty tensors -- Ht = 0 -- as NULL)."""
    for l, (ws, (ht, hc)) in enumerate(zip(w.layers, w.hidden)):
        ly = t.layers[l]
        for name in _LAYER_FIELDS:
            v = ws.get(name)
            setattr(ly, name, v.data_ptr() if v is not None and v.numel() else None)
        ly.tok_hidden, ly.ch_hidden = ht, hc
        t.ch_w1T[l], t.ch_w2T[l] = ws['ch_w1T'].data_ptr(), ws['ch_w2T'].data_ptr()
    for name in ('tw', 'tb', 'proj_w2T', 'w0T_time', 'w0T_pair0', 'w0T_pair1', 'rp_w2T'):
        v = w.head.get(name)
        setattr(t, name, v.data_ptr() if v is not None and v.numel() else None)


def _run(t, dev) -> None:
    """The backward over the filled block ``t``: the one call, or its launches one by one."""
    if mode() == 'py':
        backward_per_launch(t, dev)
        return
    lib = _native.load()
    need = int(lib.tgmx_tpnet_backward_workspace_bytes(ctypes.byref(t)))
    if need == 0:
        _native.check(-1, 'tgmx_tpnet_backward_workspace_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need
    _native.check(lib.tgmx_tpnet_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_tpnet_backward')
    t.workspace, t.workspace_bytes = None, 0


def token_grad_views(buf: Tensor, K: int, Ht: int) -> List[Tensor]:
    """The six token-block gradients as views of one partial-sum row, in ``tgmx_mixer_layer_t``'s order (tok_g, tok_b, tok_w1, tok_b1, tok_w2, tok_b2)."""
    KH = K * Ht
    w2, w1 = buf[:KH].view(K, Ht), buf[KH : 2 * KH].view(Ht, K)
    o = 2 * KH
    b2, tb, tg, b1 = buf[o : o + K], buf[o + K : o + 2 * K], buf[o + 2 * K : o + 3 * K], buf[o + 3 * K : o + 3 * K + Ht]
    return [tg, tb, w1, b1, w2, b2]


# ---- TPNet ---------------------------------------------------------------------------------------------------------------------------------------
class TPNetFunction(torch.autograd.Function):
    """``params``: every parameter of the module in ``parameters()`` order."""

    @staticmethod
    def forward(ctx, module, a: dict, *params):
        lib = _native.load()
        blk, _ = module._weights()
        B, k, L, dev = a['B'], a['k'], module.num_layers, a['node_x'].device
        d = module._dims()
        R = 2 * B * k
        R2 = 2 * R if d['od'] else 0
        drop = next_drop(module, module.dropout)
        # what the backward reads stays in buffers this call owns; pf, y, h, z1 and the last z are the module's scratch
        feat, feat_h, x0, hp, save_z, save_z1 = _grad_views([(R2, d['ldf']), (R2, d['ldfh']), (R, d['ldx0']), (R, d['ldhp']), (L, R * d['ldz']), (L, R * d['ldz'])], dev)
        lg = torch.empty(R, dtype=torch.float64, device=dev)
        _, _, pf, _, _, z, z1, y, h = module._scratch(B, k, dev)
        out = torch.empty((2 * B, module.output_dim), dtype=torch.float32, device=dev)
        module._bind_inputs(blk, a)
        blk.feat, blk.feat_h, blk.pf, blk.x0, blk.hp = feat.data_ptr(), feat_h.data_ptr(), pf.data_ptr(), x0.data_ptr(), hp.data_ptr()
        blk.z, blk.z1, blk.y, blk.h = z.data_ptr(), z1.data_ptr(), y.data_ptr(), h.data_ptr()
        blk.ldf, blk.ldfh, blk.ldx0, blk.ldhp, blk.ldz, blk.ldh = d['ldf'], d['ldfh'], d['ldx0'], d['ldhp'], d['ldz'], d['ldh']
        blk.out = out.data_ptr()
        save = _native.TPNetSave(save_z.data_ptr(), save_z1.data_ptr(), lg.data_ptr())
        check_supported(lib.tgmx_tpnet_forward_train(ctypes.byref(blk), ctypes.byref(save), _native.dropout_desc(*drop), _native.stream_ptr()),
                        'tgmx_tpnet_forward_train')  # fmt: skip
        # the weights belong to THIS forward: a later parameter version rebuilds the module's cache, not what the call holds
        w = backward_weights(module)
        ctx.module = module
        ctx.s = SimpleNamespace(B=B, k=k, dims=d, drop=drop, eps=float(blk.eps), feat=feat, feat_h=feat_h, x0=x0, hp=hp, save_z=save_z, save_z1=save_z1, lg=lg, w=w)
        return out[:B], out[B:]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_src: Optional[Tensor], g_dst: Optional[Tensor]):
        module, s = ctx.module, ctx.s
        params = param_list(module)
        need = dict(zip((id(p) for p in params), ctx.needs_input_grad[2:]))
        dev, B, E, K, d = s.x0.device, s.B, module.output_dim, s.k, s.dims
        zero = lambda: torch.zeros((B, E), dtype=torch.float32, device=dev)
        g = _rows(torch.cat([zero() if g_src is None else g_src.float(), zero() if g_dst is None else g_dst.float()], dim=0))
        t = _native.TPNetBwd()
        t.B, t.k, t.dN, t.dE, t.dT, t.E, t.od, t.num_layers = B, K, module.node_feat_dim, module.edge_x_dim, module.time_feat_dim, E, d['od'], module.num_layers
        t.eps = s.eps
        t.drop_p, t.drop_seed, t.drop_stream = s.drop
        t.g, t.ldg = g.data_ptr(), g.stride(0)
        t.feat, t.feat_h, t.x0, t.hp, t.lg = s.feat.data_ptr(), s.feat_h.data_ptr(), s.x0.data_ptr(), s.hp.data_ptr(), s.lg.data_ptr()
        t.save_z, t.save_z1 = s.save_z.data_ptr(), s.save_z1.data_ptr()
        t.ldf, t.ldfh, t.ldx0, t.ldhp, t.ldz, t.ldh = d['ldf'], d['ldfh'], d['ldx0'], d['ldhp'], d['ldz'], d['ldh']
        _fill_weights(t, s.w)
        by_id = {}
        heads = _head_params(module)
        views = _grad_views([tuple(p.shape) if p is not None else (0,) for p in heads], dev)
        for name, p, v in zip(_HEAD_FIELDS, heads, views):
            if p is not None and need[id(p)] and v.numel():
                setattr(t, name, v.data_ptr())
                by_id[id(p)] = v
        keep = []
        for l, m in enumerate(module.mlp_mixers):
            ps = _layer_params(m)
            ht = s.w.hidden[l][0]
            if any(need[id(p)] for p in ps[:6]):  # one buffer, one colsum: all six or none
                buf = torch.empty(max(1, part_floats(K, ht)), dtype=torch.float32, device=dev)
                keep.append(buf)
                t.d_tok[l] = buf.data_ptr()
                for p, v in zip(ps[:6], token_grad_views(buf, K, ht)):
                    by_id[id(p)] = v
            ch = _grad_views([tuple(p.shape) for p in ps[6:]], dev)
            for name, p, v in zip(_CH_FIELDS, ps[6:], ch):
                if need[id(p)]:
                    setattr(t.d_layers[l], name, v.data_ptr())
                    by_id[id(p)] = v
        _run(t, dev)
        return (None, None) + tuple(by_id.get(id(p)) if n else None for p, n in zip(params, ctx.needs_input_grad[2:]))


def apply(module, a: dict) -> Tuple[Tensor, Tensor]:
    """The encoder's training path: (z_src, z_dst) with ``grad_fn`` = :class:`TPNetFunction`."""
    return TPNetFunction.apply(module, a, *param_list(module))


# ---- the launches of tgmx_tpnet_backward, one ctypes call each (TGMX_TPNET_BWD=py) ---------------------------------------------------------------
def _ch_wanted(d) -> bool:
    return any(getattr(d, n) for n in _CH_FIELDS)


def backward_per_launch(a, dev) -> None:
    """What ``tgmx_tpnet_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here."""
    Q, K, E, L, od, dT = 2 * a.B, a.k, a.E, a.num_layers, a.od, a.dT
    R, W = Q * K, a.dN + a.dT + a.dE + 2 * a.od
    ldz, ldhp, ldf, ldfh, ldt = a.ldz, a.ldhp, a.ldf, a.ldfh, up4(dT)
    # the channel block is GraphMixer's: its launches read the block through GraphMixer's field names
    view = SimpleNamespace(S=Q, K=K, D=E, E=2 * E, num_layers=L, layers=a.layers, d_layers=a.d_layers, ch_w1T=a.ch_w1T, ch_w2T=a.ch_w2T, save_z1=a.save_z1,
                           ldz=ldz, ldh=a.ldh, eps=a.eps, drop_p=a.drop_p, drop_seed=a.drop_seed, drop_stream=a.drop_stream)
    run = _LayerRun(view, dev)
    lib, st = run.lib, run.st
    Ht = max([a.layers[l].tok_hidden for l in range(L)] + [0])
    run.cs_ws = run.buf(256 * max(2 * E, part_floats(K, Ht), 4 * od, dT, 1, *[a.layers[l].ch_hidden for l in range(L)]))
    want_rp1 = bool(od and (a.d_rp_w1 or a.d_rp_b1))
    want_rp = bool(od and (want_rp1 or a.d_rp_w2 or a.d_rp_b2))
    want_time = bool(dT and (a.d_tw or a.d_tb))
    want_hp = bool(a.d_proj_w0 or a.d_proj_b0 or want_rp or want_time)
    want_proj = bool(want_hp or a.d_proj_w2 or a.d_proj_b2)
    lowest = 0 if want_proj else next((l for l in range(L) if a.d_tok[l] or _ch_wanted(a.d_layers[l])), L)
    if not want_proj and lowest == L:
        return
    # 1. the token mean
    gz = run.buf(R * ldz)
    _native.check(lib.tgmx_tpnet_mean_backward(a.g, a.ldg, Q, K, E, gz, ldz, st), 'tgmx_tpnet_mean_backward')
    # 2. the layers, last first
    ldp = up4(part_floats(K, Ht))
    for l in range(L - 1, lowest - 1, -1):
        ly = a.layers[l]
        tok = bool(a.d_tok[l])
        du = run.channel(l, gz, tok or l > lowest or want_proj)
        if du is None:
            return
        site = [_native.dropout_desc(a.drop_p, a.drop_seed, a.drop_stream + 4 * l + s) for s in range(2)]
        dx, part = run.buf(R * ldz), (run.buf(Q * ldp) if tok else None)
        check_supported(lib.tgmx_tpnet_token_backward(a.save_z + l * 4 * R * ldz, ldz, du, ldz, Q, K, E, ly.tok_g, ly.tok_b, ly.tok_w1, ly.tok_b1, ly.tok_hidden,
                                                      ly.tok_w2, a.eps, dx, ldz, part, ldp, site[0], site[1], st), 'tgmx_tpnet_token_backward')  # fmt: skip
        if tok:
            run.colsum(part, ldp, Q, part_floats(K, ly.tok_hidden), a.d_tok[l])
        gz = dx
    if not want_proj:
        return
    # 3. the projection
    if a.d_proj_w2:
        run.tn(gz, ldz, a.hp, ldhp, a.d_proj_w2, 2 * E, R, E, 2 * E)
    if a.d_proj_b2:
        run.colsum(gz, ldz, R, E, a.d_proj_b2)
    if not want_hp:
        return
    dhp = run.buf(R * ldhp)
    run.nt(gz, ldz, a.proj_w2T, E, dhp, ldhp, R, 2 * E, E)
    _native.check(lib.tgmx_relu_mask(dhp, ldhp, a.hp, ldhp, R, 2 * E, st), 'tgmx_relu_mask')
    if a.d_proj_w0:
        run.tn(dhp, ldhp, a.x0, a.ldx0, a.d_proj_w0, W, R, 2 * E, W)
    if a.d_proj_b0:
        run.colsum(dhp, ldhp, R, 2 * E, a.d_proj_b0)
    # 4. the time encoder
    if want_time:
        dtime, trows = run.buf(R * ldt), run.buf(R * 2 * dT)
        run.nt(dhp, ldhp, a.w0T_time, 2 * E, dtime, ldt, R, dT, 2 * E)
        _native.check(lib.tgmx_tpnet_time_backward(dtime, ldt, a.lg, R, a.tw, a.tb, dT, trows, st), 'tgmx_tpnet_time_backward')
        if a.d_tw:
            run.colsum(trows, 2 * dT, R, dT, a.d_tw)
        if a.d_tb:
            run.colsum(trows + 4 * dT, 2 * dT, R, dT, a.d_tb)
    # 5. the pair-feature MLP
    if want_rp:
        dpf = run.buf(2 * R * ldf)
        run.nt(dhp, ldhp, a.w0T_pair0, 2 * E, dpf, ldf, R, od, 2 * E)
        run.nt(dhp, ldhp, a.w0T_pair1, 2 * E, dpf + 4 * R * ldf, ldf, R, od, 2 * E)
        if a.d_rp_w2:
            run.tn(dpf, ldf, a.feat_h, ldfh, a.d_rp_w2, 4 * od, 2 * R, od, 4 * od)
        if a.d_rp_b2:
            run.colsum(dpf, ldf, 2 * R, od, a.d_rp_b2)
        if want_rp1:
            dfh = run.buf(2 * R * ldfh)
            run.nt(dpf, ldf, a.rp_w2T, od, dfh, ldfh, 2 * R, 4 * od, od)
            _native.check(lib.tgmx_relu_mask(dfh, ldfh, a.feat_h, ldfh, 2 * R, 4 * od, st), 'tgmx_relu_mask')
            if a.d_rp_w1:
                run.tn(dfh, ldfh, a.feat, ldf, a.d_rp_w1, od, 2 * R, 4 * od, od)
            if a.d_rp_b1:
                run.colsum(dfh, ldfh, 2 * R, 4 * od, a.d_rp_b1)


__all__ = ['DEFAULT', 'TPNetFunction', 'apply', 'backward_per_launch', 'backward_weights', 'in_envelope', 'mode', 'part_floats', 'token_grad_views',
           'train_supported']
