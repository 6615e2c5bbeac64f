"""Training path of ``GraphMixerEncoder`` and ``MLPMixer`` (examples/linkproppred/graphmixer.py and tgm/nn/modules/mlp_mixer.py under
``loss.backward()``): a ``torch.autograd.Function`` whose forward is the inference call in its saving form (``tgmx_graphmixer_forward_train``:
the same kernels in the same order, so with dropout off the grad-enabled forward returns the bits of the no-grad one) and whose backward is
ONE native call (``tgmx_graphmixer_backward``, ``csrc/mixer_bwd.hip``), with g = dL/dout [S, E]:

    the output layer              -> d out_w = g^T cat (``tgmx_sgemm_tn``), d out_b (``tgmx_colsum``), dcat = g out_w[:, :D] (``tgmx_sgemm_nt_ep``)
    the link mean                 -> ``tgmx_mixer_tail_backward``: gz[s, k] = dcat[s] / max(1, valid_s) on the valid slots, 0 on the pads
    per layer, last first:
      y, a = y W1^T + b1          -> recomputed: ``tgmx_mixer_channel_norm`` on the saved z1, the forward's GEMM without its GELU
      dh = drop3(gz) W2           -> ``tgmx_sgemm_nt_ep`` on the transposed weight (``tgmx_dropout`` first when p > 0)
      hd, da                      -> ``tgmx_mixer_gelu_backward``: exact-erf GELU' with site 2's mask, in place
      d W2, d b2, d W1, d b1      -> ``tgmx_sgemm_tn``, ``tgmx_colsum``
      dy = da W1, LN_C backward   -> ``tgmx_sgemm_nt_ep``, ``tgmx_ln_backward``; d channel_norm.* by ``tgmx_colsum``; dz1 = du + gz (``tgmx_add_cols``)
      the token block             -> ``tgmx_mixer_token_backward``: gz <- dx, and per column the rows whose sums (two ``tgmx_sgemm_tn``, four
                                     ``tgmx_colsum`` over S C rows) are d token_norm.* and d token_feedforward.ffn.{0,3}.*
    the projection                -> d proj_w = gz^T x0, d proj_b

No gradient goes to ``node_feat``, the edge features or the (frozen) time encoder: a call that asks for one is outside the envelope and
keeps the composed path, as does ``TGMX_GRAPHMIXER_BWD=torch``.  ``TGMX_GRAPHMIXER_BWD=py`` issues the backward's launches one ctypes call
each from :func:`backward_per_launch` -- the readable specification, the same bits.  Every sum has a fixed order (the dense library's
contracts; no float atomics): two runs give the same bits.

What is saved: the RECOMPUTING form.  Kept per call, in buffers the call owns: ``x0`` (the projection's input), per layer the token block's
input ``z`` and its output ``z1``, ``cat``, and the caller's ``nbr_nids``; ``y`` and the channel FFN's pre-activations are recomputed (one
small kernel and one GEMM per layer).  Bytes per call, float32, R = S K rows, leading dimensions rounded up to 4 floats:

    x0        4 R (D + T)
    z | z1    8 num_layers R D
    cat       4 S (D + F)

-- at the cfg-2 shape (bs 200: S = 600, K = 20, R = 12 000, D = 172, T = F = 100, 2 layers) 13.1 MB of x0, 33.0 MB of z | z1 and 0.65 MB
of cat.  Keeping the pre-activations as well would add 4 R Hc = 33 MB a layer and save one GEMM a layer; that form is not built (it has
to be shown faster first).  The weights the backward reads -- and the transposes of the channel FFN's and the output layer's -- are
copied once per parameter version by ``tgmx_pack2d`` (:func:`backward_weights`) and bound to the call at FORWARD time: forward A,
optimizer step, forward B, backward B, backward A differentiates A with A's weights.

Dropout (train mode, p > 0): four sites per layer l with ``tgmx_dropout_t`` masks, seed ``torch.initial_seed()``, stream
``call * 64 + 4 l + site`` (0 token hidden [S, C, Ht], 1 token output [S, C, K], 2 channel hidden [S K, Hc], 3 channel output [S K, C];
the element index is the flat index in the site's tensor), regenerated in the backward, never stored.
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
from ._paramver import TransientCaches, param_key, param_list

DEFAULT = 'native'  # chosen by tools/bench_graphmixer_train.py against the composed path
_LAYER_FIELDS = ('tok_g', 'tok_b', 'tok_w1', 'tok_b1', 'tok_w2', 'tok_b2', 'ch_g', 'ch_b', 'ch_w1', 'ch_b1', 'ch_w2', 'ch_b2')


def mode() -> str:
    """'native', 'py' or 'torch': ``TGMX_GRAPHMIXER_BWD``, anything else is the default."""
    m = os.environ.get('TGMX_GRAPHMIXER_BWD', '')
    return m if m in ('native', 'py', 'torch') else DEFAULT


def train_supported(K: int, C: int, Ht: int) -> bool:
    """A seed's tile fits both token kernels' LDS (``tgmx_mixer_train_supported``: the one function the forward and the backward go by)."""
    return bool(_native.load().tgmx_mixer_train_supported(int(K), int(C), int(Ht)))


def _layer_params(m) -> tuple:
    """The twelve parameters of an ``MLPMixer`` in ``tgmx_mixer_layer_t``'s order."""
    tf, cf = m.token_feedforward.ffn, m.channel_feedforward.ffn
    return (m.token_norm.weight, m.token_norm.bias, tf[0].weight, tf[0].bias, tf[3].weight, tf[3].bias,
            m.channel_norm.weight, m.channel_norm.bias, cf[0].weight, cf[0].bias, cf[3].weight, cf[3].bias)  # fmt: skip


def _mixer_ok(m, p: float) -> bool:
    """``_check_native()`` passes, the four dropout sites share ``p`` and the tile fits the token kernels."""
    try:
        m._check_native()
    except NotImplementedError:
        return False
    tf, cf = m.token_feedforward.ffn, m.channel_feedforward.ffn
    if not 0.0 <= float(p) < 1.0 or any(float(d.p) != float(p) for d in (tf[2], tf[4], cf[2], cf[4])) or cf[0].out_features < 1:
        return False
    return train_supported(m.num_tokens, m.num_channels, tf[0].out_features)


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


def in_envelope(module, node_feat: Tensor, nbr_edge_x: Tensor, S: int) -> bool:
    """The native training path takes this ``GraphMixerEncoder.forward`` call (the conditions of the module docstring)."""
    if S <= 0 or node_feat.requires_grad or nbr_edge_x.requires_grad or not _common(module, node_feat, nbr_edge_x):
        return False
    if any(p.requires_grad for p in module.time_encoder.parameters()):
        return False
    eps = {float(n.eps) for m in module.mlp_mixers for n in (m.token_norm, m.channel_norm)}
    return len(eps) <= 1 and all(_mixer_ok(m, module.dropout) for m in module.mlp_mixers)


def mixer_in_envelope(mixer, x: Tensor) -> bool:
    """The native training path takes this ``MLPMixer.forward`` call: as above, for one block; ``x`` may ask for its gradient."""
    return x.shape[0] > 0 and _common(mixer, x) and _mixer_ok(mixer, mixer.dropout)


def next_drop(module, p: float) -> Tuple[float, int, int]:
    """(p, seed, first stream) of this forward call's dropout sites; (0, 0, 0) when dropout is off."""
    if not (module.training and p > 0):
        return (0.0, 0, 0)
    d = module.__dict__
    d['_tgmx_drop_calls'] = d.get('_tgmx_drop_calls', 0) + 1
    return (float(p), torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, d['_tgmx_drop_calls'] * 64)


def _site(drop: Tuple[float, int, int], layer: int, site: int):
    return _native.dropout_desc(drop[0], drop[1], drop[2] + 4 * layer + site)


# ---- the weights of a call -------------------------------------------------------------------------------------------------------------------
def backward_weights(owner, mixers, out_w: Optional[Tensor], D: int) -> SimpleNamespace:
    """What the backward reads of the parameters, copied by ``tgmx_pack2d`` and cached on ``owner`` against their versions: per mixer the
    ``tgmx_mixer_layer_t`` fields it needs, ``ch_w1T`` [C, Hc] and ``ch_w2T`` [Hc, C]; ``out_wT`` [D, E] (the link columns of
    ``output_layer.weight``).  A call keeps the object it got at forward time."""
    d = owner.__dict__
    # (param_list caches on the module, and only TransientCaches modules leave that cache behind on pickle / deepcopy)
    key = param_key(owner if isinstance(owner, TransientCaches) else tuple(owner.parameters()))
    if d.get('_tgmx_gm_wkey') == key:
        return d['_tgmx_gm_w']
    dev = next(owner.parameters()).device
    plan = []  # (name, layer, source, transpose)
    for l, m in enumerate(mixers):
        ps = _layer_params(m)
        for name, p in zip(_LAYER_FIELDS, ps):
            if name not in ('tok_b2', 'ch_w2', 'ch_b2'):  # (the backward reads neither the second Linears' biases nor W2 itself)
                plan.append((name, l, p.detach(), False))
        plan += [('ch_w1T', l, ps[8].detach(), True), ('ch_w2T', l, ps[10].detach(), True)]
    if out_w is not None:
        plan.append(('out_wT', 0, out_w.detach()[:, :D], True))
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
    w = SimpleNamespace(layers=[dict() for _ in mixers], out_wT=None, views=views,
                        hidden=[(m.token_feedforward.ffn[0].out_features, m.channel_feedforward.ffn[0].out_features) for m in mixers])
    for (name, l, t, tr), v in zip(plan, views):
        if name == 'out_wT':
            w.out_wT = v
        else:
            w.layers[l][name] = v
    d['_tgmx_gm_w'], d['_tgmx_gm_wkey'] = w, key
    return w


def _fill_layers(t, w: SimpleNamespace) -> None:
    """``t.layers`` / ``t.ch_w1T`` / ``t.ch_w2T`` from the call's weights (empty tensors -- Ht = 0 -- as NULL)."""
    for l, (ws, (ht, hc)) in enumerate(zip(w.layers, w.hidden)):
        ly = t.layers[l]
        for name in _LAYER_FIELDS:
            v = ws.get(name)
            setattr(ly, name, v.data_ptr() if v is not None and v.numel() else None)
        ly.tok_hidden, ly.ch_hidden = ht, hc
        t.ch_w1T[l], t.ch_w2T[l] = ws['ch_w1T'].data_ptr(), ws['ch_w2T'].data_ptr()


def _run(t, dev) -> None:
    """The backward over the filled block ``t``: the one call, or its launches one by one."""
    if mode() == 'py':
        backward_per_launch(t, dev)
        return
    lib = _native.load()
    need = int(lib.tgmx_graphmixer_backward_workspace_bytes(ctypes.byref(t)))
    if need == 0:
        _native.check(-1, 'tgmx_graphmixer_backward_workspace_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need
    _native.check(lib.tgmx_graphmixer_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_graphmixer_backward')
    t.workspace, t.workspace_bytes = None, 0


def _layer_grads(m, need: List[bool], dev) -> Tuple[List[Optional[Tensor]], list]:
    """(the twelve gradients of a mixer in ``tgmx_mixer_layer_t``'s order, None where not wanted;  their pointers, NULL where not wanted or
    empty)."""
    ps = _layer_params(m)
    views = _grad_views([tuple(p.shape) for p in ps], dev)
    grads = [v if n else None for v, n in zip(views, need)]
    return grads, [g.data_ptr() if g is not None and g.numel() else None for g in grads]


# ---- GraphMixerEncoder ---------------------------------------------------------------------------------------------------------------------------
class GraphMixerFunction(torch.autograd.Function):
    """``params``: every parameter of the module in ``parameters()`` order."""

    @staticmethod
    def forward(ctx, module, a: dict, *params):
        lib = _native.load()
        blk, _ = module._weights()
        S, L, dev = a['S'], module.num_layers, a['ex'].device
        d = module._dims(S)
        R, ldx0, ldz, ldcat = d['R'], d['ldx0'], d['ldz'], d['ldcat']
        drop = next_drop(module, module.dropout)
        # what the backward reads stays in buffers this call owns; y, h and the last z are the module's scratch
        x0, cat, save_z, save_z1 = _grad_views([(R, ldx0), (S, ldcat), (L, R * ldz), (L, R * ldz)], dev)
        _, z, z1, y, h, _ = module._scratch(S, dev)
        out = torch.empty((S, module.embed_dim), dtype=torch.float32, device=dev)
        blk.nbr_edge_x, blk.seed_t, blk.nbr_t, blk.nbr_nids = a['ex'].data_ptr(), a['seed_t'].data_ptr(), a['nbr_t'].data_ptr(), a['nids'].data_ptr()
        for g, t in enumerate(a['seeds']):
            blk.seeds[g], blk.n_seeds[g] = t.data_ptr(), t.numel()
        blk.tg_nbr, blk.tg_lo, blk.tg_cnt = a['tg_nbr'].data_ptr(), a['tg_lo'].data_ptr(), a['tg_cnt'].data_ptr()
        blk.node_x, blk.num_nodes, blk.S = a['node_x'].data_ptr(), a['node_x'].shape[0], S
        blk.x0, blk.z, blk.z1, blk.y, blk.h, blk.cat = x0.data_ptr(), z.data_ptr(), z1.data_ptr(), y.data_ptr(), h.data_ptr(), cat.data_ptr()
        blk.ldx0, blk.ldz, blk.ldh, blk.ldcat = ldx0, ldz, d['ldh'], ldcat
        blk.out = out.data_ptr()
        check_supported(lib.tgmx_graphmixer_forward_train(ctypes.byref(blk), save_z.data_ptr(), save_z1.data_ptr(), _native.dropout_desc(*drop),
                                                          _native.stream_ptr()), 'tgmx_graphmixer_forward_train')  # fmt: skip
        # the weights belong to THIS forward: a later parameter version (forward A, optimizer step, forward B, backward B, backward A)
        # rebuilds the module's cache, not what the call holds
        w = backward_weights(module, module.mlp_mixers, module.output_layer.weight, module.edge_dim)
        ctx.module = module
        ctx.s = SimpleNamespace(S=S, dims=d, drop=drop, x0=x0, cat=cat, save_z=save_z, save_z1=save_z1, nids=a['nids'], w=w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        module, s = ctx.module, ctx.s
        params = param_list(module)
        need = dict(zip((id(p) for p in params), ctx.needs_input_grad[2:]))
        dev = s.x0.device
        g = _rows(g)
        K, D, T, E, F_ = module.num_tokens, module.edge_dim, module.time_dim, module.embed_dim, module.node_dim
        pl, ol = module.projection_layer, module.output_layer
        t = _native.GraphMixerBwd()
        t.S, t.K, t.D, t.T, t.E, t.F, t.num_layers = s.S, K, D, T, E, F_, module.num_layers
        t.eps = float(module.mlp_mixers[0].token_norm.eps) if module.num_layers else 1e-5
        t.drop_p, t.drop_seed, t.drop_stream = s.drop
        t.g, t.ldg = g.data_ptr(), g.stride(0)
        t.x0, t.save_z, t.save_z1, t.cat, t.nbr_nids = s.x0.data_ptr(), s.save_z.data_ptr(), s.save_z1.data_ptr(), s.cat.data_ptr(), s.nids.data_ptr()
        t.ldx0, t.ldz, t.ldh, t.ldcat = s.dims['ldx0'], s.dims['ldz'], s.dims['ldh'], s.dims['ldcat']
        _fill_layers(t, s.w)
        t.out_wT = s.w.out_wT.data_ptr()
        by_id = {}
        heads = _grad_views([(D, D + T), (D,), (E, D + F_), (E,)], dev)
        for name, p, v in zip(('d_proj_w', 'd_proj_b', 'd_out_w', 'd_out_b'), (pl.weight, pl.bias, ol.weight, ol.bias), heads):
            if need[id(p)]:
                setattr(t, name, v.data_ptr())
                by_id[id(p)] = v
        for l, m in enumerate(module.mlp_mixers):
            ps = _layer_params(m)
            grads, ptrs = _layer_grads(m, [need[id(p)] for p in ps], dev)
            for name, p, gr, ptr in zip(_LAYER_FIELDS, ps, grads, ptrs):
                setattr(t.d_layers[l], name, ptr)
                by_id[id(p)] = gr
        _run(t, dev)
        return (None, None) + tuple(by_id.get(id(p)) if n else None for p, n in zip(params, ctx.needs_input_grad[2:]))


def apply(module, a: dict) -> Tensor:
    """The encoder's training path: ``out`` with ``grad_fn`` = :class:`GraphMixerFunction`."""
    return GraphMixerFunction.apply(module, a, *param_list(module))


# ---- MLPMixer alone ------------------------------------------------------------------------------------------------------------------------------
class MixerFunction(torch.autograd.Function):
    """One ``MLPMixer`` block on x [B, K, C]: the forward's launches and the layer part of :func:`backward_per_launch`, one ctypes call each."""

    @staticmethod
    def forward(ctx, mixer, x: Tensor, *params):
        from .mlp_mixer import sgemm_ep

        lib, st = _native.load(), _native.stream_ptr()
        xin = x.detach().contiguous()
        B, K, C = xin.shape
        R, dev = B * K, xin.device
        tn, cn, tf, cf = mixer.token_norm, mixer.channel_norm, mixer.token_feedforward.ffn, mixer.channel_feedforward.ffn
        Hc = cf[0].out_features
        drop = next_drop(mixer, mixer.dropout)
        z1, y, h = _grad_views([(R, C), (R, C), (R, Hc)], dev)
        out = torch.empty((B, K, C), dtype=torch.float32, device=dev)
        check_supported(
            lib.tgmx_mixer_token_train(xin.data_ptr(), C, B, K, C, tn.weight.data_ptr(), tn.bias.data_ptr(), tf[0].weight.data_ptr(), tf[0].bias.data_ptr(),
                                       tf[0].out_features, tf[3].weight.data_ptr(), tf[3].bias.data_ptr(), cn.weight.data_ptr(), cn.bias.data_ptr(),
                                       float(tn.eps), z1.data_ptr(), y.data_ptr(), C, _site(drop, 0, 0), _site(drop, 0, 1), st),
            'tgmx_mixer_token_train',
        )  # fmt: skip
        sgemm_ep(y, cf[0].weight.detach(), h, cf[0].bias.detach(), act=2)
        o2 = out.view(R, C)
        if not drop[0]:
            sgemm_ep(h, cf[3].weight.detach(), o2, cf[3].bias.detach(), res=z1)
        else:
            _native.check(lib.tgmx_dropout(h.data_ptr(), Hc, R, Hc, _site(drop, 0, 2), h.data_ptr(), Hc, st), 'tgmx_dropout')
            sgemm_ep(h, cf[3].weight.detach(), o2, cf[3].bias.detach())
            _native.check(lib.tgmx_dropout(o2.data_ptr(), C, R, C, _site(drop, 0, 3), o2.data_ptr(), C, st), 'tgmx_dropout')
            _native.check(lib.tgmx_add_cols(o2.data_ptr(), C, z1.data_ptr(), C, R, C, 1, st), 'tgmx_add_cols')
        ctx.mixer, ctx.params = mixer, params
        ctx.s = SimpleNamespace(B=B, K=K, C=C, drop=drop, x=xin, z1=z1, w=backward_weights(mixer, [mixer], None, C))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        mixer, s = ctx.mixer, ctx.s
        B, K, C, dev = s.B, s.K, s.C, s.x.device
        R = B * K
        g = g if g.dtype == torch.float32 else g.float()
        g = g.contiguous().view(R, C)
        ps = _layer_params(mixer)
        order = {id(p): i for i, p in enumerate(ps)}
        params, need_p = ctx.params, ctx.needs_input_grad[2:]
        need = [False] * 12
        for p, n in zip(params, need_p):
            need[order[id(p)]] = n
        t = _native.GraphMixerBwd()
        t.S, t.K, t.D, t.num_layers, t.eps = B, K, C, 1, float(mixer.token_norm.eps)
        t.drop_p, t.drop_seed, t.drop_stream = s.drop
        t.save_z, t.save_z1, t.ldz, t.ldh = s.x.data_ptr(), s.z1.data_ptr(), C, s.w.hidden[0][1]
        _fill_layers(t, s.w)
        grads, ptrs = _layer_grads(mixer, need, dev)
        for name, ptr in zip(_LAYER_FIELDS, ptrs):
            setattr(t.d_layers[0], name, ptr)
        dx = _LayerRun(t, dev).layer(0, g, want_dx=ctx.needs_input_grad[1])
        return (None, dx.view(B, K, C) if ctx.needs_input_grad[1] else None) + tuple(grads[order[id(p)]] if n else None for p, n in zip(params, need_p))


def apply_mixer(mixer, x: Tensor) -> Tensor:
    """``MLPMixer``'s training path: ``out`` with ``grad_fn`` = :class:`MixerFunction`."""
    return MixerFunction.apply(mixer, x, *mixer.parameters())


# ---- the launches of tgmx_graphmixer_backward, one ctypes call each (TGMX_GRAPHMIXER_BWD=py) -----------------------------------------------------
def _wanted(d, names) -> bool:
    return any(getattr(d, n) for n in names)


class _LayerRun:
    """The buffers of ``tgmx_graphmixer_backward``'s workspace as tensors, and one layer's launches in its order with its kernels."""

    def __init__(self, a, dev) -> None:
        self.a, self.dev, self.keep = a, dev, []
        self.lib, self.st = _native.load(), _native.stream_ptr()
        self.R, self.SC = a.S * a.K, a.S * a.D
        Ht = max([a.layers[l].tok_hidden for l in range(a.num_layers)] + [0])
        self.ldw = up4(4 * a.K + 2 * Ht)
        self.cs_ws = self.buf(256 * max([a.E, a.D, a.K, Ht, 1] + [a.layers[l].ch_hidden for l in range(a.num_layers)]))

    def buf(self, n: int) -> int:
        self.keep.append(torch.empty(max(1, n), dtype=torch.float32, device=self.dev))
        return self.keep[-1].data_ptr()

    def tn(self, A, lda, B, ldb, C, ldc, R, M, N) -> None:
        ws = self.buf(self.lib.tgmx_sgemm_tn_workspace_bytes(R, M, N, 1) // 4 + 1)
        _native.check(self.lib.tgmx_sgemm_tn(A, lda, B, ldb, C, ldc, R, M, N, 1, 0, 0, 0, 0, ws, self.st), 'tgmx_sgemm_tn')

    def colsum(self, src, ld, R, C, dst) -> None:
        _native.check(self.lib.tgmx_colsum(src, ld, R, C, dst, 0, self.cs_ws, self.st), 'tgmx_colsum')

    def nt(self, A, lda, B, ldb, C, ldc, M, N, K, bias=None) -> None:
        _native.check(self.lib.tgmx_sgemm_nt_ep(A, lda, B, ldb, C, ldc, M, N, K, bias, 0, None, 0, self.st), 'tgmx_sgemm_nt_ep')

    def channel(self, l: int, gz: int, down: bool) -> Optional[int]:
        """The channel block of layer ``l`` (``mixer_channel_backward``) given the pointer of gz [R, ldz]: writes the block's wanted gradients;
        returns the pointer of dz1 [R, ldz] = the LayerNorm's backward + the residual, or None when nobody reads it (``down`` false)."""
        a, lib, st, R = self.a, self.lib, self.st, self.R
        D, ldz, ldh = a.D, a.ldz, a.ldh
        ly, d = a.layers[l], a.d_layers[l]
        hc = ly.ch_hidden
        z1 = a.save_z1 + l * 4 * R * ldz
        site = [_native.dropout_desc(a.drop_p, a.drop_seed, a.drop_stream + 4 * l + s) for s in range(4)]
        abuf, hbuf, y = self.buf(R * ldh), self.buf(R * ldh), self.buf(R * ldz)
        _native.check(lib.tgmx_mixer_channel_norm(z1, ldz, R, D, ly.ch_g, ly.ch_b, a.eps, y, ldz, st), 'tgmx_mixer_channel_norm')
        self.nt(y, ldz, ly.ch_w1, D, abuf, ldh, R, hc, D, ly.ch_b1)
        g3 = gz
        if a.drop_p > 0:
            g3 = self.buf(R * ldz)
            _native.check(lib.tgmx_dropout(gz, ldz, R, D, site[3], g3, ldz, st), 'tgmx_dropout')
        self.nt(g3, ldz, a.ch_w2T[l], D, hbuf, ldh, R, hc, D)
        _native.check(lib.tgmx_mixer_gelu_backward(abuf, ldh, hbuf, ldh, R, hc, site[2], st), 'tgmx_mixer_gelu_backward')
        if d.ch_w2:
            self.tn(g3, ldz, abuf, ldh, d.ch_w2, hc, R, D, hc)
        if d.ch_b2:
            self.colsum(g3, ldz, R, D, d.ch_b2)
        if d.ch_w1:
            self.tn(hbuf, ldh, y, ldz, d.ch_w1, D, R, hc, D)
        if d.ch_b1:
            self.colsum(hbuf, ldh, R, hc, d.ch_b1)
        if not (d.ch_g or d.ch_b or down):
            return None
        dy, du, dgx = self.buf(R * ldz), self.buf(R * ldz), self.buf(R * ldz)
        self.keep.append(torch.zeros(ldz, dtype=torch.float32, device=self.dev))  # (the native call clears its row with a memset)
        zero = self.keep[-1].data_ptr()
        self.nt(hbuf, ldh, a.ch_w1T[l], hc, dy, ldz, R, D, hc)
        _native.check(lib.tgmx_ln_backward(dy, ldz, z1, ldz, zero, 0, ly.ch_g, D, a.eps, R, du, ldz, dgx, ldz, st), 'tgmx_ln_backward')
        if d.ch_g:
            self.colsum(dgx, ldz, R, D, d.ch_g)
        if d.ch_b:
            self.colsum(dy, ldz, R, D, d.ch_b)
        if not down:
            return None
        _native.check(lib.tgmx_add_cols(du, ldz, gz, ldz, R, D, 1, st), 'tgmx_add_cols')
        return du

    def layer(self, l: int, gz, want_dx: bool):
        """Layer ``l`` given gz = the gradient at its output (a tensor [R, ldz] or its pointer): writes the layer's wanted gradients;
        returns the gradient at its input (a tensor [R, ldz]), or None when nobody reads it (``want_dx`` false, no token gradient wanted)."""
        a, lib, st, R, SC, ldw = self.a, self.lib, self.st, self.R, self.SC, self.ldw
        K, D, ldz = a.K, a.D, a.ldz
        ly, d = a.layers[l], a.d_layers[l]
        ht = ly.tok_hidden
        gz = gz.data_ptr() if torch.is_tensor(gz) else gz
        z_in = a.save_z + l * 4 * R * ldz
        tok = _wanted(d, _LAYER_FIELDS[:6])
        site = [_native.dropout_desc(a.drop_p, a.drop_seed, a.drop_stream + 4 * l + s) for s in range(4)]
        du = self.channel(l, gz, tok or want_dx)
        if du is None:
            return None
        # the token block
        dx = torch.empty((R, ldz), dtype=torch.float32, device=self.dev)
        rows = self.buf(SC * ldw) if tok else None
        check_supported(lib.tgmx_mixer_token_backward(z_in, ldz, du, ldz, a.S, K, D, ly.tok_g, ly.tok_b, ly.tok_w1, ly.tok_b1, ht, ly.tok_w2, a.eps,
                                                      dx.data_ptr(), ldz, rows, ldw, site[0], site[1], st), 'tgmx_mixer_token_backward')  # fmt: skip
        if tok:
            r_do, r_xn, r_dxn, r_gxh, r_hd, r_da = (rows + 4 * o for o in (0, K, 2 * K, 3 * K, 4 * K, 4 * K + ht))
            if ht > 0:
                if d.tok_w2:
                    self.tn(r_do, ldw, r_hd, ldw, d.tok_w2, ht, SC, K, ht)
                if d.tok_w1:
                    self.tn(r_da, ldw, r_xn, ldw, d.tok_w1, K, SC, ht, K)
                if d.tok_b1:
                    self.colsum(r_da, ldw, SC, ht, d.tok_b1)
            if d.tok_b2:
                self.colsum(r_do, ldw, SC, K, d.tok_b2)
            if d.tok_b:
                self.colsum(r_dxn, ldw, SC, K, d.tok_b)
            if d.tok_g:
                self.colsum(r_gxh, ldw, SC, K, d.tok_g)
        return dx


def backward_per_launch(a, dev) -> None:
    """What ``tgmx_graphmixer_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here."""
    run = _LayerRun(a, dev)
    lib, st = run.lib, run.st
    S, K, D, T, E, F_, L, R, ldz = a.S, a.K, a.D, a.T, a.E, a.F, a.num_layers, run.R, a.ldz
    # 1. the output layer
    if a.d_out_w:
        run.tn(a.g, a.ldg, a.cat, a.ldcat, a.d_out_w, D + F_, S, E, D + F_)
    if a.d_out_b:
        run.colsum(a.g, a.ldg, S, E, a.d_out_b)
    want_proj = bool(a.d_proj_w or a.d_proj_b)
    lowest = 0 if want_proj else next((l for l in range(L) if _wanted(a.d_layers[l], _LAYER_FIELDS)), L)
    if not want_proj and lowest == L:
        return
    # 2. the link mean
    dcat = run.buf(S * ldz)
    gz = torch.empty((R, ldz), dtype=torch.float32, device=dev)
    run.nt(a.g, a.ldg, a.out_wT, E, dcat, ldz, S, D, E)
    _native.check(lib.tgmx_mixer_tail_backward(dcat, ldz, a.nbr_nids, S, K, D, gz.data_ptr(), ldz, st), 'tgmx_mixer_tail_backward')
    # 3. the layers, last first
    for l in range(L - 1, lowest - 1, -1):
        gz = run.layer(l, gz, want_dx=l > lowest or want_proj)
        if gz is None:
            return
    # 4. the projection
    if a.d_proj_w:
        run.tn(gz.data_ptr(), ldz, a.x0, a.ldx0, a.d_proj_w, D + T, R, D, D + T)
    if a.d_proj_b:
        run.colsum(gz.data_ptr(), ldz, R, D, a.d_proj_b)


__all__ = ['DEFAULT', 'GraphMixerFunction', 'MixerFunction', 'apply', 'apply_mixer', 'backward_per_launch', 'backward_weights', 'in_envelope',
           'mixer_in_envelope', 'mode', 'next_drop', 'train_supported']
