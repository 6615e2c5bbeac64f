"""Training path of ``DyGFormer`` and ``TransformerEncoder`` (examples/linkproppred/dygformer.py and tgm/nn/encoder/dygformer.py under
``loss.backward()``): a ``torch.autograd.Function`` whose forward is the inference call in its saving form (``tgmx_dygformer_forward_train``:
the same kernels in the same order, so with dropout off the grad-enabled forward returns the bits of the no-grad one) and whose backward is
ONE native call (``tgmx_dygformer_backward``, ``csrc/dygformer_bwd.hip``), with g = dL/dout [2 P, E]:

    the output layer              -> d out_w = g^T mean (``tgmx_sgemm_tn``), d out_b (``tgmx_colsum``), dmean = g out_w (``tgmx_sgemm_nt_ep``)
    the patch mean                -> ``tgmx_dygformer_mean_backward``: gz[(2 p + side) Np + t] = dmean[side P + p] / Np
    per layer, last first (``tgmx_dygformer_layer_backward``):
      y = LN1(x1), a = y W1^T + b1  -> recomputed: ``tgmx_layernorm_rows`` on the saved x1, the forward's GEMM without its GELU
      dh = drop3(gz) W2           -> ``tgmx_sgemm_nt_ep`` on the transposed weight (``tgmx_dropout`` first when p > 0)
      hd, da                      -> ``tgmx_mixer_gelu_backward``: exact-erf GELU' with site 2's mask, in place
      d W2, d b2, d W1, d b1      -> ``tgmx_sgemm_tn``, ``tgmx_colsum``
      dy = da W1, LN1 backward    -> ``tgmx_sgemm_nt_ep``, ``tgmx_ln_backward``; d norm_layers.1.* by ``tgmx_colsum``; dx1 = du + gz
      d out_proj.*, datt          -> from drop1(dx1): ``tgmx_sgemm_tn``, ``tgmx_colsum``, ``tgmx_sgemm_nt_ep``
      dqkv                        -> ``tgmx_mha_small_backward``: the probabilities recomputed in LDS from the saved qkv, site 0's mask
      d in_proj_*, LN0 backward   -> y = LN0(x) recomputed; ``tgmx_sgemm_tn``, ``tgmx_colsum``, ``tgmx_sgemm_nt_ep``, ``tgmx_ln_backward``; gz <- du + dx1
    the four projections          -> d proj_w[c] = gz[:, c C : (c + 1) C]^T ch[c] (un-padded), d proj_b[c]
    the time tail                 -> dtime = gz_time proj_w[time]; ``tgmx_dygformer_time_backward``; d time_encoder.w.* by ``tgmx_colsum``
    the co-occurrence tail        -> dfeat = gz_co proj_w[co]; ``tgmx_dygformer_cooccurrence_backward`` (one-hot counts through ``tgmx_sgemm_tn``,
                                     then the table's own backward over its L + 1 rows)

No gradient goes to ``node_x`` or the edge features: a call that asks for one is outside the envelope and keeps the composed path, as does
``TGMX_DYGFORMER_BWD=torch``.  ``TGMX_DYGFORMER_BWD=py`` issues the backward's launches one ctypes call each from
:func:`backward_per_launch` -- the readable specification, the same bits (the co-occurrence tail stays one call: its three small kernels
have no entry points of their own).  Every sum has a fixed order (no float atomics): two runs give the same bits.

What is saved: the RECOMPUTING form.  Kept per call, in buffers the call owns: the four channel inputs ``ch[c]``, the co-occurrence
counts, per layer its input ``x``, ``qkv``, ``att`` and ``x1``, the last layer's output and the patch means; ``y = LN(.)`` and the FFN's
pre-activations are recomputed (two LayerNorm launches and one GEMM per layer).  Bytes per call, float32, n = 2 P L slots, R = 2 P Np
token rows, D = 4 C, leading dimensions rounded up to 4 floats:

    ch        4 n (dN + dE + dT + C)
    counts    8 n
    x         4 (num_layers + 1) R D
    qkv       12 num_layers R D
    att | x1  8 num_layers R D
    mean      8 P D

-- at the example's shape (bs 200: P = 200, L = 32, patch 1, R = n = 12 800, dN = 128, dE = 172, dT = 100, C = 50, D = 200, 2 layers) 23.1 MB
of ch, 30.7 MB of x, 61.4 MB of qkv and 41.0 MB of att | x1: 61.4 MB a layer, 156.6 MB a call.  The weights the backward reads -- and the
transposes it multiplies by -- are copied once per parameter version by ``tgmx_pack2d`` (:func:`backward_weights`) and bound to the call
at FORWARD time: forward A, optimizer step, forward B, backward B, backward A differentiates A with A's weights.

Dropout (train mode, p > 0): four sites per layer l with ``tgmx_dropout_t`` masks, seed ``torch.initial_seed()``, stream
``call * 64 + 4 l + site`` (0 attention probabilities [P, H, T, T], 1 the attention block's output [R, D] before the residual, 2 the
FFN's hidden activations [R, 4 D], 3 the FFN's output [R, D] before the residual; the element index is the flat index in the site's
tensor), regenerated in the backward, never stored.

The attention backward keeps Q, K, V, dO and two T x T tiles resident in LDS (140.5 KiB at T = 64, dh = 100: one workgroup per CU), so
the training envelope is narrower than inference's: ``tgmx_mha_small_train_supported`` (T = 64 with dh = 128 and T = 128 with dh = 32
are outside and compose).
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
from ._gclstm_train import _grad_views
from ._graphmixer_train import next_drop
from ._paramver import TransientCaches, param_key, param_list
from .time_encoding import Time2Vec

DEFAULT = 'native'  # chosen by tools/bench_dygformer_train.py against the composed path
_LAYER_FIELDS = ('ln0_g', 'ln0_b', 'in_w', 'in_b', 'out_w', 'out_b', 'ln1_g', 'ln1_b', 'w1', 'b1', 'w2', 'b2')
_TR_FIELDS = (('in_wT', 'in_w'), ('out_wT', 'out_w'), ('w1T', 'w1'), ('w2T', 'w2'))
_READ = ('ln0_g', 'ln0_b', 'ln1_g', 'ln1_b', 'w1', 'b1')  # what tgmx_dygformer_layer_backward reads of tgmx_dygformer_layer_t


def mode() -> str:
    """'native', 'py' or 'torch': ``TGMX_DYGFORMER_BWD``, anything else is the default."""
    m = os.environ.get('TGMX_DYGFORMER_BWD', '')
    return m if m in ('native', 'py', 'torch') else DEFAULT


def train_supported(T: int, dh: int) -> bool:
    """T tokens at head dimension dh fit the attention backward's LDS plan (``tgmx_mha_small_train_supported``: the one function the
    forward's path choice and the backward go by)."""
    return bool(_native.load().tgmx_mha_small_train_supported(int(T), int(dh)))


def _layer_params(t) -> tuple:
    """The twelve parameters of a ``TransformerEncoder`` in ``tgmx_dygformer_layer_t``'s order."""
    mha, ln, lin = t.multi_head_attention, t.norm_layers, t.linear_layers
    return (ln[0].weight, ln[0].bias, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, ln[1].weight, ln[1].bias,
            lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias)  # fmt: skip


def _layer_ok(t, p: float) -> bool:
    """The packed in-projection with bias, one eps, and the layer's ``nn.Dropout`` and its attention's ``dropout`` both equal ``p``."""
    mha = t.multi_head_attention
    if mha.in_proj_weight is None or mha.in_proj_bias is None or mha.bias_k is not None or mha.batch_first or mha.out_proj.bias is None:
        return False
    if t.norm_layers[0].eps != t.norm_layers[1].eps or any(n.weight is None or n.bias is None for n in t.norm_layers):
        return False
    return 0.0 <= float(p) < 1.0 and float(t.dropout.p) == float(p) and float(mha.dropout) == float(p)


def _common(module, *inputs: Tensor) -> bool:
    """Gradients on with a parameter that wants one, no autocast, not ``torch`` mode, float32 inputs and contiguous float32 parameters on
    one device."""
    dev = inputs[0].device
    if mode() == 'torch' or not torch.is_grad_enabled() or torch.is_autocast_enabled(dev.type):
        return False
    if any(t.device != dev or t.dtype != torch.float32 for t in inputs):
        return False
    params = list(module.parameters())
    if any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
        return False
    return any(p.requires_grad for p in params)


def in_envelope(module, a: dict) -> bool:
    """The native training path takes this ``DyGFormer`` call (the conditions of the module docstring of ``dygformer.py``)."""
    node_x, nbr_x = a['node_x'], a['nbr_x']
    if a['P'] <= 0 or node_x.requires_grad or nbr_x.requires_grad or not _common(module, node_x, nbr_x):
        return False
    if type(module.time_encoder) is not Time2Vec or not module._native_ok(a['L']):
        return False
    D = module.num_channels * module.channel_embedding_dim
    if D % module.num_heads or not train_supported(2 * module.num_patches, D // module.num_heads):
        return False
    eps = {float(n.eps) for t in module.transformers for n in t.norm_layers}
    return len(eps) <= 1 and all(_layer_ok(t, module.dropout) for t in module.transformers)


def layer_in_envelope(t, x: Tensor) -> bool:
    """The native training path takes this ``TransformerEncoder.forward`` call: as above, for one layer; ``x`` may ask for its gradient."""
    B, T, D = x.shape
    return B * T > 0 and _common(t, x) and _layer_ok(t, t.dropout_rate) and D % t.num_heads == 0 and train_supported(T, D // t.num_heads)


def _site0(drop: Tuple[float, int, int], layer: int):
    """The descriptor a layer's entry points take: its four sites draw from stream + 0 .. 3."""
    return _native.dropout_desc(drop[0], drop[1], drop[2] + 4 * layer)


# ---- the weights of a call -------------------------------------------------------------------------------------------------------------------
def _pack(plan, dev) -> List[Tensor]:
    """``plan``: (source 2-D view, transpose, rows the destination is zero-padded to).  One ``tgmx_pack2d`` launch per 32 copies."""
    shapes = []
    for src, tr, pad_rows in plan:
        r, c = (src.shape[1], src.shape[0]) if tr else tuple(src.shape)
        shapes.append((max(r, pad_rows), c))
    views = _grad_views(shapes, dev)
    jobs = []
    for (src, tr, _), v in zip(plan, views):
        if v.numel() == 0:
            continue
        rows, cols = (src.shape[1], src.shape[0]) if tr else tuple(src.shape)
        j = _native.PackJob()
        j.src, j.dst, j.src_ld, j.dst_ld, j.rows, j.cols, j.dst_rows, j.dst_cols, j.transpose = src.data_ptr(), v.data_ptr(), src.stride(0), v.shape[1], rows, cols, v.shape[0], v.shape[1], int(tr)
        jobs.append(j)
    lib, st = _native.load(), _native.stream_ptr()
    for i in range(0, len(jobs), 32):  # TGMX_PACK_MAX_JOBS
        chunk = (_native.PackJob * len(jobs[i : i + 32]))(*jobs[i : i + 32])
        _native.check(lib.tgmx_pack2d(chunk, len(chunk), st), 'tgmx_pack2d')
    return views


def _as2d(p: Tensor) -> Tensor:
    p = p.detach()
    return p if p.dim() == 2 else p.view(1, -1)


def backward_weights(owner, layers, model=None) -> SimpleNamespace:
    """What the backward reads of the parameters, copied by ``tgmx_pack2d`` and cached on ``owner`` against their versions: per layer the
    ``tgmx_dygformer_layer_t`` fields it reads and the four transposes; for the whole model also ``out_wT`` [D, E], the padded transposes
    ``proj_wT`` [patch ldch, C] of the time and co-occurrence projections, the time encoder and the co-occurrence encoder's first Linear
    and ``co_w2T``.  A call keeps the object it got at forward time."""
    d = owner.__dict__
    key = param_key(owner if isinstance(owner, TransientCaches) else tuple(owner.parameters()))
    if d.get('_tgmx_dyg_wkey') == key:
        return d['_tgmx_dyg_w']
    dev = next(owner.parameters()).device
    plan, names = [], []
    for l, t in enumerate(layers):
        ps = dict(zip(_LAYER_FIELDS, _layer_params(t)))
        for n in _READ:
            plan.append((_as2d(ps[n]), False, 0))
            names.append((l, n))
        for n, src in _TR_FIELDS:
            plan.append((_as2d(ps[src]), True, 0))
            names.append((l, n))
    if model is not None:
        C, ps_, dd = model.channel_embedding_dim, model.patch_size, model._dims()
        co, tw = model.co_occurrence_encoder.neighbor_co_occurrence_encoder, model.time_encoder.w
        plan.append((_as2d(model.output_layer.weight), True, 0))
        names.append((-1, 'out_wT'))
        for n, p in (('tw', tw.weight.reshape(-1)), ('tb', tw.bias), ('co_w1', co[0].weight.reshape(-1)), ('co_b1', co[0].bias)):
            plan.append((_as2d(p), False, 0))
            names.append((-1, n))
        plan.append((_as2d(co[2].weight), True, 0))
        names.append((-1, 'co_w2T'))
        for c, dc in ((2, model.time_feat_dim), (3, C)):  # slot s of a patch: rows [s ldch, s ldch + dc) of the transpose, zero rows up to ldch
            w = model.projection_layer[model.CHANNELS[c]].weight.detach()
            for s in range(ps_):
                plan.append((w[:, s * dc : (s + 1) * dc], True, dd['ldch'][c]))
                names.append((-1, ('proj_wT', c, s)))
    views = _pack(plan, dev)
    w = SimpleNamespace(layers=[dict() for _ in layers], views=views, model={})
    for (l, n), v in zip(names, views):
        (w.layers[l] if l >= 0 else w.model)[n] = v
    if model is not None:
        # the per-slot pieces were carved next to each other only up to the 256-byte grid: one contiguous [patch ldch, C] per channel
        for c in (2, 3):
            parts = [w.model.pop(('proj_wT', c, s)) for s in range(model.patch_size)]
            w.model[f'proj_wT{c}'] = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    d['_tgmx_dyg_w'], d['_tgmx_dyg_wkey'] = w, key
    return w


def _fill_layer(ly, tr, ws: dict) -> None:
    for n in _READ:
        setattr(ly, n, ws[n].data_ptr())
    for n, _ in _TR_FIELDS:
        setattr(tr, n, ws[n].data_ptr())


def _layer_grads(t, need: List[bool], dev) -> Tuple[List[Optional[Tensor]], list]:
    """(the twelve gradients of a layer in ``tgmx_dygformer_layer_t``'s order, None where not wanted;  their pointers, NULL where not wanted)."""
    views = _grad_views([tuple(p.shape) for p in _layer_params(t)], dev)
    grads = [v if n else None for v, n in zip(views, need)]
    return grads, [g.data_ptr() if g is not None else None for g in grads]


# ---- DyGFormer -------------------------------------------------------------------------------------------------------------------------------
class DyGFormerFunction(torch.autograd.Function):
    """``params``: every parameter of the module in ``parameters()`` order.  Returns (src_emb, dst_emb)."""

    @staticmethod
    def forward(ctx, module, a: dict, *params):
        lib = _native.load()
        blk, _ = module._weights()
        P, L, dev, nL = a['P'], a['L'], a['node_x'].device, module.num_layers
        d = module._dims()
        ldch, ldx, ldq, ldh = d['ldch'], d['ldx'], d['ldq'], d['ldh']
        n, R = 2 * P * L, 2 * P * module.num_patches
        drop = next_drop(module, module.dropout)
        # what the backward reads stays in buffers this call owns; table, y and h are the module's scratch
        bufs = _grad_views([(n, ld) for ld in ldch] + [(2 * P, ldx), (nL + 1, R * ldx), (nL, R * ldq), (nL, R * ldx), (nL, R * ldx)], dev)
        ch, (mean, save_x, save_qkv, save_att, save_x1) = bufs[:4], bufs[4:]
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
        scratch = module._scratch(P, L, dev)
        out = torch.empty((2 * P, module.output_dim), dtype=torch.float32, device=dev)
        blk.node_x, blk.num_nodes = a['node_x'].data_ptr(), a['node_x'].shape[0]
        blk.src, blk.dst, blk.edge_time, blk.P = a['src'].data_ptr(), a['dst'].data_ptr(), a['t'].data_ptr(), P
        blk.nbr_nids, blk.nbr_t, blk.nbr_x, blk.S = a['nids'].data_ptr(), a['nbr_t'].data_ptr(), a['nbr_x'].data_ptr(), a['nids'].shape[0]
        blk.src_rows, blk.dst_rows = _native.ptr(a['src_rows']), _native.ptr(a['dst_rows'])
        blk.table = scratch[0].data_ptr()
        for c in range(4):
            blk.ch[c], blk.ldch[c] = ch[c].data_ptr(), ldch[c]
        blk.x, blk.y, blk.x1, blk.att, blk.qkv, blk.h = (b.data_ptr() for b in scratch[5:11])
        blk.mean = mean.data_ptr()
        blk.ldx, blk.ldq, blk.ldh = ldx, ldq, ldh
        blk.out = out.data_ptr()
        save = _native.DyGFormerSave(counts.data_ptr(), save_x.data_ptr(), save_qkv.data_ptr(), save_att.data_ptr(), save_x1.data_ptr())
        check_supported(lib.tgmx_dygformer_forward_train(ctypes.byref(blk), ctypes.byref(save), _native.dropout_desc(*drop), _native.stream_ptr()),
                        'tgmx_dygformer_forward_train')  # fmt: skip
        # the weights belong to THIS forward: a later parameter version rebuilds the module's cache, not what the call holds
        w = backward_weights(module, module.transformers, module)
        ctx.module = module
        ctx.s = SimpleNamespace(P=P, L=L, dims=d, drop=drop, ch=ch, counts=counts, mean=mean, save_x=save_x, save_qkv=save_qkv, save_att=save_att,
                                save_x1=save_x1, w=w, eps=float(blk.eps), a={k: a[k] for k in ('src', 'dst', 't', 'nids', 'nbr_t', 'src_rows', 'dst_rows')})  # fmt: skip
        return out[:P], out[P:]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_src: Optional[Tensor], g_dst: Optional[Tensor]):
        module, s = ctx.module, ctx.s
        params = param_list(module)
        need = dict(zip((id(p) for p in params), ctx.needs_input_grad[2:]))
        dev, P, E = s.mean.device, s.P, module.output_dim
        z = lambda: torch.zeros((P, E), dtype=torch.float32, device=dev)
        g = torch.cat([z() if g_src is None else g_src.float(), z() if g_dst is None else g_dst.float()], dim=0)
        C, ps = module.channel_embedding_dim, module.patch_size
        t = _native.DyGFormerBwd()
        t.P, t.S, t.k, t.dN, t.dE, t.dT = P, s.a['nids'].shape[0], s.L - 1, module.node_feat_dim, module.edge_x_dim, module.time_feat_dim
        t.C, t.patch, t.heads, t.E, t.num_layers, t.eps = C, ps, module.num_heads, E, module.num_layers, s.eps
        t.drop_p, t.drop_seed, t.drop_stream = s.drop
        t.src, t.dst, t.edge_time, t.nbr_nids, t.nbr_t = (s.a[k].data_ptr() for k in ('src', 'dst', 't', 'nids', 'nbr_t'))
        t.src_rows, t.dst_rows = _native.ptr(s.a['src_rows']), _native.ptr(s.a['dst_rows'])
        t.g, t.ldg = g.data_ptr(), g.stride(0)
        for c in range(4):
            t.ch[c], t.ldch[c] = s.ch[c].data_ptr(), s.dims['ldch'][c]
        t.counts, t.mean = s.counts.data_ptr(), s.mean.data_ptr()
        t.save_x, t.save_qkv, t.save_att, t.save_x1 = s.save_x.data_ptr(), s.save_qkv.data_ptr(), s.save_att.data_ptr(), s.save_x1.data_ptr()
        t.ldx, t.ldq, t.ldh = s.dims['ldx'], s.dims['ldq'], s.dims['ldh']
        for l, ws in enumerate(s.w.layers):
            _fill_layer(t.layers[l], t.tr[l], ws)
        m = s.w.model
        t.out_wT, t.tw, t.tb, t.co_w1, t.co_b1, t.co_w2T = (m[k].data_ptr() for k in ('out_wT', 'tw', 'tb', 'co_w1', 'co_b1', 'co_w2T'))
        t.proj_wT[2], t.proj_wT[3] = m['proj_wT2'].data_ptr(), m['proj_wT3'].data_ptr()
        by_id = {}
        co, tw, pl, ol = module.co_occurrence_encoder.neighbor_co_occurrence_encoder, module.time_encoder.w, module.projection_layer, module.output_layer
        heads = [('d_tw', tw.weight), ('d_tb', tw.bias), ('d_co_w1', co[0].weight), ('d_co_b1', co[0].bias), ('d_co_w2', co[2].weight),
                 ('d_co_b2', co[2].bias), ('d_out_w', ol.weight), ('d_out_b', ol.bias)]  # fmt: skip
        projs = [pl[n] for n in module.CHANNELS]
        views = _grad_views([tuple(p.shape) for _, p in heads] + [tuple(p.weight.shape) for p in projs] + [tuple(p.bias.shape) for p in projs], dev)
        for (name, p), v in zip(heads, views):
            if need[id(p)]:
                setattr(t, name, v.data_ptr())
                by_id[id(p)] = v
        for c, p in enumerate(projs):
            if need[id(p.weight)]:
                t.d_proj_w[c] = views[8 + c].data_ptr()
                by_id[id(p.weight)] = views[8 + c]
            if need[id(p.bias)]:
                t.d_proj_b[c] = views[12 + c].data_ptr()
                by_id[id(p.bias)] = views[12 + c]
        for l, tr in enumerate(module.transformers):
            ps_ = _layer_params(tr)
            grads, ptrs = _layer_grads(tr, [need[id(p)] for p in ps_], dev)
            for name, p, gr, ptr in zip(_LAYER_FIELDS, ps_, grads, ptrs):
                setattr(t.d_layers[l], name, ptr)
                by_id[id(p)] = gr
        _run(t, dev)
        return (None, None) + tuple(by_id.get(id(p)) if n else None for p, n in zip(params, ctx.needs_input_grad[2:]))


def apply(module, a: dict) -> Tuple[Tensor, Tensor]:
    """The encoder's training path: (src_emb, dst_emb) with ``grad_fn`` = :class:`DyGFormerFunction`."""
    return DyGFormerFunction.apply(module, a, *param_list(module))


def _run(t, dev) -> None:
    """The backward over the filled block ``t``: the one call, or its launches one by one."""
    if mode() == 'py':
        backward_per_launch(t, dev)
        return
    lib = _native.load()
    need = int(lib.tgmx_dygformer_backward_workspace_bytes(ctypes.byref(t)))
    if need == 0:
        _native.check(-1, 'tgmx_dygformer_backward_workspace_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need
    _native.check(lib.tgmx_dygformer_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_dygformer_backward')
    t.workspace, t.workspace_bytes = None, 0


# ---- TransformerEncoder alone ----------------------------------------------------------------------------------------------------------------
class LayerFunction(torch.autograd.Function):
    """One ``TransformerEncoder`` on x [B, T, D]: ``tgmx_dygformer_layer_train`` and ``tgmx_dygformer_layer_backward`` (or its launches)."""

    @staticmethod
    def forward(ctx, t, x: Tensor, *params):
        from .dygformer import _layer_block
        from ._fwd_plumbing import weight_keeper

        lib, st = _native.load(), _native.stream_ptr()
        B, T, D = x.shape
        R, dev, ldx, ldq, ldh = B * T, x.device, up4(D), up4(3 * D), 4 * D
        xin = torch.zeros((R, ldx), dtype=torch.float32, device=dev)
        xin[:, :D] = x.detach().reshape(R, D)
        drop = next_drop(t, t.dropout_rate)
        xout, y, x1, att, qkv, h = _grad_views([(R, ldx)] * 4 + [(R, ldq), (R, ldh)], dev)
        keep, f32 = weight_keeper()
        ly = _layer_block(t, f32)
        check_supported(
            lib.tgmx_dygformer_layer_train(ctypes.byref(ly), B, T, t.num_heads, D, float(t.norm_layers[0].eps), xin.data_ptr(), xout.data_ptr(), y.data_ptr(),
                                           x1.data_ptr(), att.data_ptr(), ldx, qkv.data_ptr(), ldq, h.data_ptr(), ldh, _site0(drop, 0), st),
            'tgmx_dygformer_layer_train',
        )  # fmt: skip
        ctx.t, ctx.params = t, params
        ctx.s = SimpleNamespace(B=B, T=T, D=D, drop=drop, x=xin, x1=x1, att=att, qkv=qkv, w=backward_weights(t, [t]))
        return xout[:, :D].reshape(B, T, D)

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        t, s = ctx.t, ctx.s
        B, T, D, dev = s.B, s.T, s.D, s.x.device
        R, ldx, ldq, ldh = B * T, up4(D), up4(3 * D), 4 * D
        gz = torch.zeros((R, ldx), dtype=torch.float32, device=dev)  # (clobbered by the backward)
        gz[:, :D] = g.reshape(R, D)
        ps = _layer_params(t)
        order = {id(p): i for i, p in enumerate(ps)}
        params, need_p = ctx.params, ctx.needs_input_grad[2:]
        need = [False] * 12
        for p, n in zip(params, need_p):
            need[order[id(p)]] = n
        grads, ptrs = _layer_grads(t, need, dev)
        ly, tr, d = _native.DyGFormerLayer(), _native.DyGFormerLayerTr(), _native.DyGFormerLayerGrad()
        _fill_layer(ly, tr, s.w.layers[0])
        for name, ptr in zip(_LAYER_FIELDS, ptrs):
            setattr(d, name, ptr)
        want_dx = ctx.needs_input_grad[1]
        dx = torch.empty((R, ldx), dtype=torch.float32, device=dev) if want_dx else None
        args = (ly, tr, d, B, T, t.num_heads, D, float(t.norm_layers[0].eps), s.x.data_ptr(), s.qkv.data_ptr(), s.att.data_ptr(), s.x1.data_ptr(), ldx, ldq,
                ldh, gz.data_ptr(), _native.ptr(dx), (s.drop[0], s.drop[1], s.drop[2]))  # fmt: skip
        if mode() == 'py':
            _LayerRun(dev).layer(*args)
        else:
            _layer_native(*args, dev)
        return (None, dx[:, :D].reshape(B, T, D) if want_dx else None) + tuple(grads[order[id(p)]] if n else None for p, n in zip(params, need_p))


def apply_layer(t, x: Tensor) -> Tensor:
    """``TransformerEncoder``'s training path: ``out`` with ``grad_fn`` = :class:`LayerFunction`."""
    return LayerFunction.apply(t, x, *t.parameters())


def _layer_native(ly, tr, d, B, T, H, D, eps, x, qkv, att, x1, ldx, ldq, ldh, g, dx, drop, dev) -> None:
    lib = _native.load()
    need = int(lib.tgmx_dygformer_layer_backward_workspace_bytes(B, T, D, ldx, ldq, ldh))
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=dev)
    check_supported(
        lib.tgmx_dygformer_layer_backward(ctypes.byref(ly), ctypes.byref(tr), ctypes.byref(d), B, T, H, D, eps, x, qkv, att, x1, ldx, ldq, ldh, g, dx,
                                          _native.dropout_desc(*drop), ws.data_ptr(), need, _native.stream_ptr()),
        'tgmx_dygformer_layer_backward',
    )  # fmt: skip


# ---- the launches of tgmx_dygformer_backward, one ctypes call each (TGMX_DYGFORMER_BWD=py) ----------------------------------------------------
class _LayerRun:
    """The buffers of the native calls' workspaces as tensors, and one layer's launches in ``tgmx_dygformer_layer_backward``'s order."""

    def __init__(self, dev) -> None:
        self.dev, self.keep = dev, []
        self.lib, self.st = _native.load(), _native.stream_ptr()

    def buf(self, n: int, zero: bool = False) -> int:
        self.keep.append((torch.zeros if zero else torch.empty)(max(1, n), dtype=torch.float32, device=self.dev))
        return self.keep[-1].data_ptr()

    def tn(self, A, lda, B, ldb, C, ldc, R, M, N) -> None:
        ws = self.buf(self.lib.tgmx_sgemm_tn_workspace_bytes(R, M, N, 1) // 4 + 1)
        _native.check(self.lib.tgmx_sgemm_tn(A, lda, B, ldb, C, ldc, R, M, N, 1, 0, 0, 0, 0, ws, self.st), 'tgmx_sgemm_tn')

    def colsum(self, src, ld, R, C, dst) -> None:
        _native.check(self.lib.tgmx_colsum(src, ld, R, C, dst, 0, self.buf(256 * C), self.st), 'tgmx_colsum')

    def nt(self, A, lda, B, ldb, C, ldc, M, N, K, bias=None) -> None:
        _native.check(self.lib.tgmx_sgemm_nt_ep(A, lda, B, ldb, C, ldc, M, N, K, bias, 0, None, 0, self.st), 'tgmx_sgemm_nt_ep')

    def layer(self, ly, tr, d, B, T, H, D, eps, x, qkv, att, x1, ldx, ldq, ldh, g, dx, drop) -> None:
        """g [R, ldx] (pointer): the gradient at the layer's output, clobbered; dx (pointer or None): the gradient at its input."""
        lib, st, R = self.lib, self.st, B * T
        site = [_native.dropout_desc(drop[0], drop[1], drop[2] + s) for s in range(4)]
        ln = lambda src, gam, bet, dst: _native.check(lib.tgmx_layernorm_rows(src, ldx, R, D, gam, bet, eps, dst, ldx, st), 'tgmx_layernorm_rows')
        y, abuf, hbuf = self.buf(R * ldx), self.buf(R * ldh), self.buf(R * ldh)
        zero = self.buf(ldx, zero=True)  # (the native call clears its row with a memset)
        # the FFN
        ln(x1, ly.ln1_g, ly.ln1_b, y)
        self.nt(y, ldx, ly.w1, D, abuf, ldh, R, 4 * D, D, ly.b1)
        g3 = g
        gt = self.buf(R * ldx) if drop[0] > 0 else None
        if drop[0] > 0:
            _native.check(lib.tgmx_dropout(g, ldx, R, D, site[3], gt, ldx, st), 'tgmx_dropout')
            g3 = gt
        self.nt(g3, ldx, tr.w2T, D, hbuf, ldh, R, 4 * D, D)
        _native.check(lib.tgmx_mixer_gelu_backward(abuf, ldh, hbuf, ldh, R, 4 * D, site[2], st), 'tgmx_mixer_gelu_backward')
        if d.w2:
            self.tn(g3, ldx, abuf, ldh, d.w2, 4 * D, R, D, 4 * D)
        if d.b2:
            self.colsum(g3, ldx, R, D, d.b2)
        if d.w1:
            self.tn(hbuf, ldh, y, ldx, d.w1, D, R, 4 * D, D)
        if d.b1:
            self.colsum(hbuf, ldh, R, 4 * D, d.b1)
        attn = bool(d.ln0_g or d.ln0_b or d.in_w or d.in_b or d.out_w or d.out_b or dx)
        if not (d.ln1_g or d.ln1_b or attn):
            return
        dy, du, dgx = self.buf(R * ldx), self.buf(R * ldx), self.buf(R * ldx)
        self.nt(hbuf, ldh, tr.w1T, 4 * D, dy, ldx, R, D, 4 * D)
        _native.check(lib.tgmx_ln_backward(dy, ldx, x1, ldx, zero, 0, ly.ln1_g, D, eps, R, du, ldx, dgx, ldx, st), 'tgmx_ln_backward')
        if d.ln1_g:
            self.colsum(dgx, ldx, R, D, d.ln1_g)
        if d.ln1_b:
            self.colsum(dy, ldx, R, D, d.ln1_b)
        if not attn:
            return
        _native.check(lib.tgmx_add_cols(g, ldx, du, ldx, R, D, 1, st), 'tgmx_add_cols')
        # the attention block
        g1 = g
        if drop[0] > 0:
            _native.check(lib.tgmx_dropout(g, ldx, R, D, site[1], gt, ldx, st), 'tgmx_dropout')
            g1 = gt
        if d.out_w:
            self.tn(g1, ldx, att, ldx, d.out_w, D, R, D, D)
        if d.out_b:
            self.colsum(g1, ldx, R, D, d.out_b)
        if not (d.ln0_g or d.ln0_b or d.in_w or d.in_b or dx):
            return
        datt, dqkv = self.buf(R * ldx), self.buf(R * ldq)
        self.nt(g1, ldx, tr.out_wT, D, datt, ldx, R, D, D)
        check_supported(lib.tgmx_mha_small_backward(qkv, ldq, datt, ldx, B, T, H, D // H, dqkv, site[0], st), 'tgmx_mha_small_backward')
        if d.in_w:
            ln(x, ly.ln0_g, ly.ln0_b, y)
            self.tn(dqkv, ldq, y, ldx, d.in_w, D, R, 3 * D, D)
        if d.in_b:
            self.colsum(dqkv, ldq, R, 3 * D, d.in_b)
        if not (d.ln0_g or d.ln0_b or dx):
            return
        self.nt(dqkv, ldq, tr.in_wT, 3 * D, dy, ldx, R, D, 3 * D)
        _native.check(lib.tgmx_ln_backward(dy, ldx, x, ldx, zero, 0, ly.ln0_g, D, eps, R, du, ldx, dgx, ldx, st), 'tgmx_ln_backward')
        if d.ln0_g:
            self.colsum(dgx, ldx, R, D, d.ln0_g)
        if d.ln0_b:
            self.colsum(dy, ldx, R, D, d.ln0_b)
        if not dx:
            return
        _native.check(lib.tgmx_add_cols(dx, ldx, du, ldx, R, D, 0, st), 'tgmx_add_cols')
        _native.check(lib.tgmx_add_cols(dx, ldx, g, ldx, R, D, 1, st), 'tgmx_add_cols')


def backward_per_launch(a, dev) -> None:
    """What ``tgmx_dygformer_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here."""
    run = _LayerRun(dev)
    lib, st = run.lib, run.st
    P, L, C, E, nL = a.P, a.k + 1, a.C, a.E, a.num_layers
    Np, D, ldx = L // a.patch, 4 * C, a.ldx
    T, R, n = 2 * Np, 2 * P * Np, 2 * P * L
    dims = (a.dN, a.dE, a.dT, C)
    # 1. the output layer
    if a.d_out_w:
        run.tn(a.g, a.ldg, a.mean, ldx, a.d_out_w, D, 2 * P, E, D)
    if a.d_out_b:
        run.colsum(a.g, a.ldg, 2 * P, E, a.d_out_b)
    want_time, want_co = bool(a.d_tw or a.d_tb), bool(a.d_co_w1 or a.d_co_b1 or a.d_co_w2 or a.d_co_b2)
    want_proj = want_time or want_co or any(a.d_proj_w[c] or a.d_proj_b[c] for c in range(4))
    wanted = lambda d: any(getattr(d, f) for f in _LAYER_FIELDS)
    lowest = 0 if want_proj else next((l for l in range(nL) if wanted(a.d_layers[l])), nL)
    if not want_proj and lowest == nL:
        return
    # 2. the patch mean
    dmean, gz, gz2 = run.buf(2 * P * ldx), run.buf(R * ldx), run.buf(R * ldx)
    run.nt(a.g, a.ldg, a.out_wT, E, dmean, ldx, 2 * P, D, E)
    _native.check(lib.tgmx_dygformer_mean_backward(dmean, ldx, P, Np, D, gz, ldx, st), 'tgmx_dygformer_mean_backward')
    # 3. the layers, last first
    for l in range(nL - 1, lowest - 1, -1):
        ox, oq = 4 * l * R * ldx, 4 * l * R * a.ldq
        down = l > lowest or want_proj
        run.layer(a.layers[l], a.tr[l], a.d_layers[l], P, T, a.heads, D, a.eps, a.save_x + ox, a.save_qkv + oq, a.save_att + ox, a.save_x1 + ox, ldx, a.ldq,
                  a.ldh, gz, gz2 if down else None, (a.drop_p, a.drop_seed, a.drop_stream + 4 * l))  # fmt: skip
        gz, gz2 = gz2, gz
    if not want_proj:
        return
    # 4. the four projections
    for c in range(4):
        ld, dc = a.ldch[c], dims[c]
        if a.d_proj_w[c]:
            for s in range(a.patch):
                run.tn(gz + 4 * c * C, ldx, a.ch[c] + 4 * s * ld, a.patch * ld, a.d_proj_w[c] + 4 * s * dc, a.patch * dc, R, C, dc)
        if a.d_proj_b[c]:
            run.colsum(gz + 4 * c * C, ldx, R, C, a.d_proj_b[c])
    # 5. the time and co-occurrence tails
    if want_time:
        ldt = a.ldch[2]
        dtime, trows = run.buf(n * ldt), run.buf(n * 2 * a.dT)
        run.nt(gz + 4 * 2 * C, ldx, a.proj_wT[2], C, dtime, a.patch * ldt, R, a.patch * ldt, C)
        _native.check(lib.tgmx_dygformer_time_backward(dtime, ldt, a.src, a.dst, a.edge_time, P, a.nbr_nids, a.nbr_t, a.S, a.k, a.src_rows, a.dst_rows,
                                                       a.tw, a.tb, a.dT, trows, st), 'tgmx_dygformer_time_backward')  # fmt: skip
        if a.d_tw:
            run.colsum(trows, 2 * a.dT, n, a.dT, a.d_tw)
        if a.d_tb:
            run.colsum(trows + 4 * a.dT, 2 * a.dT, n, a.dT, a.d_tb)
    if want_co:
        ldf = a.ldch[3]
        dfeat = run.buf(n * ldf)
        run.nt(gz + 4 * 3 * C, ldx, a.proj_wT[3], C, dfeat, a.patch * ldf, R, a.patch * ldf, C)
        cooccurrence_backward(a.counts, dfeat, ldf, n, L, C, a.co_w1, a.co_b1, a.co_w2T, a.d_co_w1, a.d_co_b1, a.d_co_w2, a.d_co_b2, dev)


def cooccurrence_backward(counts, dfeat, ldf, n, L, C, w1, b1, w2T, d_w1, d_b1, d_w2, d_b2, dev) -> None:
    """``tgmx_dygformer_cooccurrence_backward`` with its workspace (all arguments device pointers or None)."""
    lib = _native.load()
    need = int(lib.tgmx_dygformer_cooccurrence_backward_workspace_bytes(n, L, C))
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=dev)
    _native.check(lib.tgmx_dygformer_cooccurrence_backward(counts, dfeat, ldf, n, L, C, w1, b1, w2T, d_w1, d_b1, d_w2, d_b2, ws.data_ptr(), need,
                                                           _native.stream_ptr()), 'tgmx_dygformer_cooccurrence_backward')  # fmt: skip


__all__ = ['DEFAULT', 'DyGFormerFunction', 'LayerFunction', 'apply', 'apply_layer', 'backward_per_launch', 'backward_weights', 'cooccurrence_backward',
           'in_envelope', 'layer_in_envelope', 'mode', 'train_supported']
