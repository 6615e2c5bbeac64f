"""Training path of the decoders: a ``torch.autograd.Function`` whose forward is ONE native call (``tgmx_decoder_forward_save``: the
head of ``tgmx_decoder_forward``, every activation the backward reads kept in buffers of THIS call) and whose backward is ONE native
call (``tgmx_decoder_backward``, ``csrc/decoder_bwd.hip``):

    the last layer, at most 16 wide     -> ``tgmx_decoder_tail_bwd`` (dx, dW, db in one pass over the rows)
    hidden Linear + ReLU layers         -> ``tgmx_sgemm_tn`` (dW), ``tgmx_colsum`` (db), ``tgmx_sgemm_nt`` on the transposed weight (dX),
                                           ``tgmx_relu_mask``
    merge stage, pair form              -> the same blocks on the two operands and the column halves of the first Linear
    merge stage, table form             -> ``tgmx_decoder_scatter`` (the pair rows summed per table row through an inverted index, no
                                           atomics), then the same blocks over the ``N'`` rows of the table

``TGMX_DECODER_BWD=py`` issues the backward's launches one ctypes call each from :func:`backward_per_launch` -- the readable
specification, the same bits; ``TGMX_DECODER_BWD=torch`` keeps the composed torch path (the heads then never come here).

The saved activations belong to the call: a training step calls one decoder for the positives and again for the negatives before one
``backward()``, so nothing the backward reads may live in the module's shared scratch buffer.  The parameters are read where they are
(the first Linear's column halves, ``lin_src`` / ``lin_dst``): nothing is stacked or transposed by torch ops per optimizer step.
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
from . import _ops
from ._fwd_plumbing import carve_scratch
from ._paramver import param_key, param_list

ACT_NONE, ACT_RELU = 0, 1


def mode() -> str:
    """'native' (default), 'py' or 'torch': ``TGMX_DECODER_BWD``."""
    m = os.environ.get('TGMX_DECODER_BWD', '')
    return m if m in ('py', 'torch') else 'native'


def _up64(n: int) -> int:
    return (n + 63) // 64 * 64


def train_weights(head, lins, kind: Optional[str]):
    """The training block with every weight pointer filled in and, per parameter of ``head`` (in ``parameters()`` order), where its gradient
    goes: cached on the head against the parameters' versions."""
    d = head.__dict__
    key = (param_key(head), kind)
    if d.get('_tgmx_twkey') == key:
        return d['_tgmx_tw']
    params = param_list(head)
    keep: list = []

    def f32(t: Tensor) -> int:
        keep.append(_ops._f32c(t.detach(), 'weight'))
        return keep[-1].data_ptr()

    w = SimpleNamespace(blk=_native.DecoderTrain(), kind=kind, keep=keep, D=0, H=0, act=ACT_NONE, slots={})
    a = w.blk.fwd
    slot = w.slots  # id(parameter) -> (field of the block, layer or None, leading dimension or None)
    if kind == 'concat':
        first, rest = lins[0], lins[1:]
        D, H = head.merge.dim, first.out_features
        p0 = f32(first.weight)
        a.wa, a.ldwa, a.wb, a.ldwb = p0, 2 * D, p0 + 4 * D, 2 * D
        a.mbias = None if first.bias is None else f32(first.bias)
        slot[id(first.weight)] = ('merge_w', None, 2 * D)
        if first.bias is not None:
            slot[id(first.bias)] = ('d_mbias', None, None)
        w.D, w.H, w.act = D, H, ACT_RELU
    elif kind == 'sum':
        rest = lins
        D = H = head.merge.dim
        src, dst = head.merge.lin_src, head.merge.lin_dst
        a.wa, a.ldwa, a.wb, a.ldwb = f32(src.weight), D, f32(dst.weight), D
        biases = [lin.bias.detach() for lin in (src, dst) if lin.bias is not None]
        a.mbias = None if not biases else f32(biases[0] if len(biases) == 1 else biases[0] + biases[1])
        slot[id(src.weight)], slot[id(dst.weight)] = ('d_wa', None, D), ('d_wb', None, D)
        if src.bias is not None:
            slot[id(src.bias)] = ('d_mbias', None, None)
        if dst.bias is not None:
            slot[id(dst.bias)] = ('d_mbias2', None, None)
        w.D, w.H, w.act = D, H, ACT_NONE
    else:
        rest = lins
        w.D = lins[0].in_features
    a.num_layers, a.merge_act, a.D, a.H, a.pool = len(rest), w.act, w.D, w.H, 0
    for l, (ly, lin) in enumerate(zip(a.layers, rest)):
        ly.w, ly.b = f32(lin.weight), (None if lin.bias is None else f32(lin.bias))
        ly.in_, ly.out = lin.in_features, lin.out_features
        slot[id(lin.weight)] = ('d_w', l, None)
        if lin.bias is not None:
            slot[id(lin.bias)] = ('d_b', l, None)
    w.dims = [(lin.in_features, lin.out_features) for lin in rest]
    w.out_dim = rest[-1].out_features
    w.params = params
    w.sizes = [_up64(p.numel()) for p in params]
    d['_tgmx_tw'], d['_tgmx_twkey'] = w, key
    return w


def _fill(w, c) -> '_native.DecoderTrain':
    """The per-call fields of the (shared, cached) block from the call's record ``c``."""
    t = w.blk
    a = t.fwd
    a.form, a.R = _native.DECODER_FORM[c.form], c.R
    a.a1, a.lda1, a.n1 = c.x1.data_ptr(), c.x1.stride(0), c.x1.shape[0]
    a.a2 = a.ia = a.ib = a.neg = a.off = a.P = a.pooled = a.pool_ws = None
    a.lda2 = a.n2 = a.idx64 = a.max_candidates = a.pool_ws_floats = 0
    a.M, a.B = -1, c.R
    a.h[0] = a.h[1] = None
    if c.form == 'pair':
        a.a2, a.lda2, a.n2 = c.x2.data_ptr(), c.x2.stride(0), c.x2.shape[0]
    elif c.form == 'table':
        a.ia, a.ib, a.idx64 = c.ia.data_ptr(), c.ib.data_ptr(), int(c.ia.dtype == torch.int64)
        a.P = _native.ptr(c.P)  # (the forward's; the backward does not read it)
    for l in range(_native.DECODER_MAX_LAYERS):
        t.act[l] = c.acts[l].data_ptr() if l < len(c.acts) and c.acts[l] is not None else None
    a.bad, a.out = c.bad.data_ptr(), c.out.data_ptr()
    return t


def _acts(w, form: str, R: int, device) -> List[Optional[Tensor]]:
    """act[0] [R, H] (None for the rows form) and act[l] [R, in_l]: views of one buffer owned by the call."""
    widths = [0 if form == 'rows' else w.H] + [i for i, _ in w.dims[1:]]
    sizes = [_up64(R * c) for c in widths]
    flat = torch.empty(max(1, sum(sizes)), dtype=torch.float32, device=device)
    return [(v[: R * c].view(R, c) if c else None) for v, c in zip(flat.split(sizes), widths)]


class DecoderFunction(torch.autograd.Function):
    """``form``: 'rows' (inputs: x), 'pair' (z_src, z_dst), 'table' (z; ``idx`` = (ia, ib) of one integer dtype).  ``shape``: the shape the
    [R, out_dim] result is returned in.  ``tensors``: the inputs, then every parameter of the head."""

    @staticmethod
    def forward(ctx, head, w, form: str, idx: Optional[Tuple[Tensor, Tensor]], shape: tuple, *tensors: Tensor) -> Tensor:
        lib = _native.load()
        x1 = tensors[0]
        dev = x1.device
        c = SimpleNamespace(form=form, x1=x1, x2=tensors[1] if form == 'pair' else None, ia=None, ib=None, P=None)
        c.R = idx[0].numel() if form == 'table' else x1.shape[0]
        if form == 'table':
            c.ia, c.ib = idx
            c.P = carve_scratch(head, [x1.shape[0] * 2 * w.H], dev)[0]
        c.acts = _acts(w, form, c.R, dev)
        c.out = torch.empty((c.R, w.out_dim), dtype=torch.float32, device=dev)
        c.bad = head._skipped(dev)
        _native.check(lib.tgmx_decoder_forward_save(ctypes.byref(_fill(w, c)), _native.stream_ptr()), 'tgmx_decoder_forward_save')
        c.P = None  # (the module's scratch: not the call's to keep)
        ctx.w, ctx.c, ctx.n_in = w, c, 2 if form == 'pair' else 1
        return c.out.view(shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout: Tensor):
        w, c = ctx.w, ctx.c
        dev = c.x1.device
        dout = dout.reshape(c.R, w.out_dim).contiguous().float()
        params = w.params
        need_in = ctx.needs_input_grad[5 : 5 + ctx.n_in]
        need_p = ctx.needs_input_grad[5 + ctx.n_in :]
        flat = torch.empty(max(1, sum(w.sizes)), dtype=torch.float32, device=dev)
        views = [v[: p.numel()].view(p.shape) for v, p in zip(flat.split(w.sizes), params)]
        t = _fill(w, c)
        t.dout, t.lddout = dout.data_ptr(), dout.stride(0)
        t.d_a1 = t.d_a2 = t.d_wa = t.d_wb = t.d_mbias = t.d_mbias2 = None
        t.ld_dwa = t.ld_dwb = 0
        for l in range(_native.DECODER_MAX_LAYERS):
            t.d_w[l] = t.d_b[l] = None
        for p, v, need in zip(params, views, need_p):
            s = w.slots.get(id(p))
            if s is None or not need:
                continue
            field, layer, ld = s
            if field == 'merge_w':  # ConcatMerge: the column halves of the first Linear's gradient
                t.d_wa, t.ld_dwa, t.d_wb, t.ld_dwb = v.data_ptr(), ld, v.data_ptr() + 4 * w.D, ld
            elif layer is not None:
                getattr(t, field)[layer] = v.data_ptr()
            else:
                setattr(t, field, v.data_ptr())
                if ld is not None:
                    setattr(t, 'ld_dwa' if field == 'd_wa' else 'ld_dwb', ld)
        d_in: List[Optional[Tensor]] = [None] * ctx.n_in
        if need_in[0]:
            d_in[0] = torch.empty((c.x1.shape[0], w.D), dtype=torch.float32, device=dev)
            t.d_a1 = d_in[0].data_ptr()
        if c.form == 'pair' and need_in[1]:
            d_in[1] = torch.empty((c.R, w.D), dtype=torch.float32, device=dev)
            t.d_a2 = d_in[1].data_ptr()
        if mode() == 'py':
            backward_per_launch(t, dev)
        else:
            lib = _native.load()
            need = int(lib.tgmx_decoder_backward_workspace_bytes(ctypes.byref(t)))
            if need == 0:
                _native.check(-1, 'tgmx_decoder_backward_workspace_bytes')
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            t.workspace, t.workspace_bytes = ws.data_ptr(), need
            _native.check(lib.tgmx_decoder_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_decoder_backward')
            t.workspace, t.workspace_bytes = None, 0
        grads = [v if (need and id(p) in w.slots) else None for p, v, need in zip(params, views, need_p)]
        return (None, None, None, None, None, *d_in, *grads)


def apply(head, lins, kind: Optional[str], form: str, idx, shape: tuple, *inputs: Tensor) -> Tensor:
    """Run the head's training path: ``inputs`` are contiguous float32 device tensors, the result comes back in ``shape``."""
    w = train_weights(head, lins, kind)
    return DecoderFunction.apply(head, w, form, idx, shape, *inputs, *w.params)


# ---- the launches of tgmx_decoder_backward, one ctypes call each (TGMX_DECODER_BWD=py) -----------------------------------------------------
def _tail_route(ly) -> bool:
    return ly.out <= _native.DECODER_MAX_TAIL and ly.out * ly.in_ * 4 <= 48 * 1024


def backward_per_launch(t, dev) -> None:
    """What ``tgmx_decoder_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here."""
    lib, st = _native.load(), _native.stream_ptr()
    a = t.fwd
    D, H, L, R, NP = a.D, a.H, a.num_layers, a.R, a.n1
    rows, table = a.form == _native.DECODER_FORM['rows'], a.form == _native.DECODER_FORM['table']
    keep: list = []

    def buf(n: int, dtype=torch.float32) -> int:
        keep.append(torch.empty(max(1, n), dtype=dtype, device=dev))
        return keep[-1].data_ptr()

    def tn(A, lda, B, ldb, C, ldc, n_rows, M, N):
        part = buf(lib.tgmx_sgemm_tn_workspace_bytes(n_rows, M, N, 1) // 4)
        _native.check(lib.tgmx_sgemm_tn(A, lda, B, ldb, C, ldc, n_rows, M, N, 1, 0, 0, 0, 0, part, st), 'tgmx_sgemm_tn')

    def colsum(X, ld, n_rows, C, out):
        _native.check(lib.tgmx_colsum(X, ld, n_rows, C, out, 0, buf(256 * C), st), 'tgmx_colsum')

    def nt(A, lda, B, ldb, C, ldc, M, N, K):
        _native.check(lib.tgmx_sgemm_nt(A, lda, B, ldb, C, ldc, M, N, K, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')

    merge_dz = bool(t.d_a1) or (not table and bool(t.d_a2))
    need_dx0 = bool(t.d_a1) if rows else (merge_dz or any(bool(p) for p in (t.d_wa, t.d_wb, t.d_mbias, t.d_mbias2)))
    widest = max([1] + [a.layers[l].in_ for l in range(L)])
    g = [buf(R * widest), buf(R * widest)]
    dout, lddout, out_dim = t.dout, t.lddout, a.layers[L - 1].out
    if table:
        clean = buf(R * out_dim)
        jobs = (_native.DropJob * (L + 1))()
        jobs[0].src, jobs[0].dst, jobs[0].lds, jobs[0].ldd, jobs[0].C = dout, clean, lddout, out_dim, out_dim
        jobs[1].src, jobs[1].dst, jobs[1].lds, jobs[1].ldd, jobs[1].C = None, t.act[0], 0, H, H
        for l in range(1, L):
            j = jobs[l + 1]
            j.src, j.dst, j.lds, j.ldd, j.C = None, t.act[l], 0, a.layers[l].in_, a.layers[l].in_
        _native.check(lib.tgmx_decoder_drop_rows(a.ia, a.ib, a.idx64, NP, R, jobs, L + 1, st), 'tgmx_decoder_drop_rows')
        dout, lddout = clean, out_dim
    wt: List[Optional[int]] = [None] * L
    wmt = None
    packs = []
    for l in range(L):
        ly = a.layers[l]
        if (l == L - 1 and _tail_route(ly)) or not (l > 0 or need_dx0):
            continue
        wt[l] = buf(ly.in_ * ly.out)
        packs.append((ly.w, wt[l], ly.in_, ly.out, ly.in_, ly.out))
    if not rows and merge_dz:
        wmt = buf(D * 2 * H)
        packs += [(a.wa, wmt, a.ldwa, 2 * H, D, H), (a.wb, wmt + 4 * H, a.ldwb, 2 * H, D, H)]
    if packs:
        jobs = (_native.PackJob * len(packs))()
        for j, (src, dst, src_ld, dst_ld, r, c_) in zip(jobs, packs):
            j.src, j.dst, j.src_ld, j.dst_ld, j.rows, j.cols, j.dst_rows, j.dst_cols, j.transpose = src, dst, src_ld, dst_ld, r, c_, r, c_, 1
        _native.check(lib.tgmx_pack2d(jobs, len(packs), st), 'tgmx_pack2d')
    dY, lddy, cur = dout, lddout, 0
    for l in range(L - 1, -1, -1):
        ly = a.layers[l]
        X = t.act[l] if l else (a.a1 if rows else t.act[0])
        ldx = ly.in_ if l else (a.lda1 if rows else H)
        x_relu = l > 0 or (not rows and a.merge_act == ACT_RELU)
        want_dx = l > 0 or need_dx0
        dX = t.d_a1 if (l == 0 and rows) else g[cur]
        if l == L - 1 and _tail_route(ly):
            floats = lib.tgmx_decoder_tail_bwd_workspace_floats(R, ly.in_, ly.out) if (t.d_w[l] or t.d_b[l]) else 0
            _native.check(lib.tgmx_decoder_tail_bwd(dY, lddy, X, ldx, R, ly.in_, ly.w, ly.out, int(x_relu), dX if want_dx else None, ly.in_, t.d_w[l],
                                                    t.d_b[l], buf(floats), floats, st), 'tgmx_decoder_tail_bwd')  # fmt: skip
        else:
            if t.d_w[l]:
                tn(dY, lddy, X, ldx, t.d_w[l], ly.in_, R, ly.out, ly.in_)
            if t.d_b[l]:
                colsum(dY, lddy, R, ly.out, t.d_b[l])
            if want_dx:
                nt(dY, lddy, wt[l], ly.out, dX, ly.in_, R, ly.in_, ly.out)
                if x_relu:
                    _native.check(lib.tgmx_relu_mask(dX, ly.in_, X, ldx, R, ly.in_, st), 'tgmx_relu_mask')
        if not want_dx:
            return
        dY, lddy, cur = dX, ly.in_, cur ^ 1
    if rows:
        return
    if t.d_mbias:
        colsum(dY, H, R, H, t.d_mbias)
    if t.d_mbias2:
        colsum(dY, H, R, H, t.d_mbias2)
    if not table:
        if t.d_wa:
            tn(dY, H, a.a1, a.lda1, t.d_wa, t.ld_dwa, R, H, D)
        if t.d_wb:
            tn(dY, H, a.a2, a.lda2, t.d_wb, t.ld_dwb, R, H, D)
        if t.d_a1:
            nt(dY, H, wmt, 2 * H, t.d_a1, D, R, D, H)
        if t.d_a2:
            nt(dY, H, wmt + 4 * H, 2 * H, t.d_a2, D, R, D, H)
    elif NP > 0 and (t.d_wa or t.d_wb or t.d_a1):
        dP = buf(NP * 2 * H)
        nbytes = lib.tgmx_decoder_scatter_workspace_bytes(R, NP, H)
        _native.check(lib.tgmx_decoder_scatter(dY, H, R, H, a.ia, a.ib, a.idx64, NP, dP, buf(nbytes, torch.uint8), nbytes, st), 'tgmx_decoder_scatter')
        if t.d_wa:
            tn(dP, 2 * H, a.a1, a.lda1, t.d_wa, t.ld_dwa, NP, H, D)
        if t.d_wb:
            tn(dP + 4 * H, 2 * H, a.a1, a.lda1, t.d_wb, t.ld_dwb, NP, H, D)
        if t.d_a1:
            nt(dP, 2 * H, wmt, 2 * H, t.d_a1, D, NP, D, 2 * H)


__all__ = ['DecoderFunction', 'apply', 'backward_per_launch', 'mode', 'train_weights']
