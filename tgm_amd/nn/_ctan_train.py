"""Training path of ``CTAN`` (tgm/nn/encoder/ctan.py under ``loss.backward()``, examples/linkproppred/ctan.py): a
``torch.autograd.Function`` whose forward is the inference call in its saving form (``tgmx_ctan_forward`` with ``x_save``: the same kernels in
the same order, so the grad-enabled forward returns the bits of the no-grad one) and whose backward is ONE native call
(``tgmx_ctan_backward``, ``csrc/ctan_bwd.hip``), with g = dL/dout:

    the final tanh                         -> ``tgmx_ctan_out_backward``: gx = g (1 - out^2)
    the edges grouped by source            -> one ``tgmx_segment_sort`` on the clamped sources, once per call
    per iteration, last first:
      q | k | v | x A^T + bias             -> the forward's batched ``tgmx_sgemm_nt`` on the saved x (recomputed: the same call, the same bits)
      dz, dq, alpha_e, s_e, d_eproj        -> ``tgmx_ctan_attend_backward``, one workgroup per target, the forward's walk twice
      dk, dv                               -> ``tgmx_ctan_source_backward``, one workgroup per source: a gather, no float atomics
      d [W_q, W_k, W_v, A], d [b_q, b_k, b_v, bias] -> one batched ``tgmx_sgemm_tn`` and one ``tgmx_colsum``, accumulating after the first
      gx <- gx + [dq | dk | dv | dz] [W_q; W_k; W_v; A] -> ``tgmx_sgemm_nt_ep`` on the transposed stacked weight, the identity as its residual
    d aconv.W = dA - dA^T                  -> ``tgmx_ctan_antisym_grad``
    d enc_x.*, d node_x                    -> ``tgmx_sgemm_tn``, ``tgmx_colsum``, ``tgmx_sgemm_nt`` (node_x only when asked)
    d lin_edge.weight, d time_enc.lin.*    -> ``tgmx_sgemm_tn``;  ``tgmx_sgemm_nt``, ``tgmx_ctan_edge_attr_backward``, ``tgmx_colsum``

Every sum has a fixed order (ascending edge id inside a wave, waves merged in wave order, the dense library's own contracts): two runs give
the same bits.  ``TGMX_CTAN_BWD=py`` issues the backward's launches one ctypes call each from :func:`backward_per_launch` -- the readable
specification, the same bits; ``TGMX_CTAN_BWD=torch`` keeps the composed torch path (``CTAN.forward_composed``).

What is saved: the RECOMPUTING form.  Kept per call are ``x`` at the entry of every iteration and what the forward produces once per call
anyway; the projections ``q | k | v | x A^T + bias``, ``tanh(z)`` and the rows' softmax state ``(m, l)`` and ``phi`` are recomputed (one
batched GEMM per iteration and a second walk in the target pass, as ``tconv_attend_backward_kernel`` does).  Bytes per call, float32 / int64:

    x_save                 4 max(num_iters, 1) U M
    edge_attr | eproj      4 E (D + T) + 4 E M
    src_ok | order | seg   8 (2 E + 2 U)
    out                    4 U M     (the caller's result, saved through autograd: an in-place write before ``backward()`` is refused)

-- at the example's shape (a bs-200 batch with 32 neighbours: U 2 099, E 5 806, M = T = 256, D = 172, 3 iterations) 6.4 MB of x and
15.9 MB of edge rows.  Keeping ``(m, l)`` and ``phi`` as well would add 4 num_iters U (M + 2) bytes and save walk 1; that form is
not built (it has to be shown faster first).  ``node_x``, ``last_update``, ``t`` are the caller's (converted) tensors; the stacked weights
are the cached copies the forward ran with, their transposes are made once per parameter version (:func:`transposed_weights`, one
``tgmx_pack2d``) and taken at FORWARD time onto the call, so a backward that runs after a later optimizer step still pairs the weights
with their own transposes; ``time_enc``'s parameters are read where they lie and saved through autograd (its version check applies).  ``msg`` gets no gradient: a call whose ``msg`` asks for one is outside the
envelope.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _native
from ._gclstm_train import _grad_views, _rows
from ._paramver import param_key, param_list

MAX_M = 256  # kCtanMaxC: one wave covers a row with four columns a lane


def mode() -> str:
    """'native' (default), 'py' or 'torch': ``TGMX_CTAN_BWD``."""
    m = os.environ.get('TGMX_CTAN_BWD', '')
    return m if m in ('py', 'torch') else 'native'


def in_envelope(module, node_x: Tensor, msg: Tensor) -> bool:
    """The native training path takes the call: float32 ``node_x`` / ``msg`` on one device, no autocast, contiguous float32 parameters there,
    at least one node, ``memory_dim`` <= 256 and no gradient asked of ``msg``."""
    if mode() == 'torch' or torch.is_autocast_enabled():
        return False
    dev = node_x.device
    if node_x.shape[0] == 0 or module.aconv.in_channels > MAX_M or msg.requires_grad:
        return False
    if any(v.device != dev or v.dtype != torch.float32 for v in (node_x, msg)):
        return False
    return not any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in param_list(module))


def transposed_weights(module, W4: Tensor):
    """(W4T [M, 4M], WxT [in_ch, M], WeT [T, M]): the stacked projections, ``enc_x.weight`` and the time columns of ``lin_edge.weight``,
    transposed by one ``tgmx_pack2d`` and cached on the module against its parameters' versions."""
    d = module.__dict__
    key = param_key(module)
    if d.get('_tgmx_ctan_wtkey') != key:
        M, T = module.aconv.in_channels, module.time_enc.out_channels
        Wx, We = module.enc_x.weight.detach(), module.aconv.phi.lin_edge.weight.detach()
        in_ch, D = Wx.shape[1], We.shape[1] - T
        dev = Wx.device
        outs = (torch.empty((M, 4 * M), dtype=torch.float32, device=dev), torch.empty((in_ch, M), dtype=torch.float32, device=dev),
                torch.empty((T, M), dtype=torch.float32, device=dev))  # fmt: skip
        jobs = (_native.PackJob * 3)()
        for j, (src, src_ld, R, C, dst) in zip(jobs, ((W4.data_ptr(), M, 4 * M, M, outs[0]), (Wx.data_ptr(), in_ch, M, in_ch, outs[1]),
                                                      (We.data_ptr() + 4 * D, D + T, M, T, outs[2]))):  # fmt: skip
            # src [R, C] (row stride src_ld) -> dst [C, R]
            j.src, j.dst, j.src_ld, j.dst_ld, j.rows, j.cols, j.dst_rows, j.dst_cols, j.transpose = src, dst.data_ptr(), src_ld, R, C, R, C, R, 1
        _native.check(_native.load().tgmx_pack2d(jobs, 3, _native.stream_ptr()), 'tgmx_pack2d')
        d['_tgmx_ctan_wt'], d['_tgmx_ctan_wtkey'] = outs, key
    return d['_tgmx_ctan_wt']


def _run(t, dev) -> None:
    """The backward over the filled block ``t``: the one call, or its launches one by one."""
    if mode() == 'py':
        backward_per_launch(t, dev)
        return
    lib = _native.load()
    need = int(lib.tgmx_ctan_backward_workspace_bytes(ctypes.byref(t)))
    if need == 0:
        _native.check(-1, 'tgmx_ctan_backward_workspace_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need
    _native.check(lib.tgmx_ctan_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_ctan_backward')
    t.workspace, t.workspace_bytes = None, 0


class CtanFunction(torch.autograd.Function):
    """``tensors``: node_x, then every parameter of the module in ``parameters()`` order."""

    @staticmethod
    def forward(ctx, module, last_update: Tensor, edge_index: Tensor, t: Tensor, msg: Tensor, *tensors):
        out, s = module._forward_native(tensors[0].detach(), last_update, edge_index, t, msg.detach(), own=True)
        # the transposes belong to the weights THIS forward ran with: a later parameter version (forward A, optimizer step, forward B,
        # backward B, backward A) rebuilds the module's cache, not what the call holds
        s.WT = transposed_weights(module, s.W4)
        ctx.module, ctx.s = module, s
        # the result itself and the time encoder's parameters, which the backward reads where they lie: autograd then refuses a backward
        # after an in-place write to any of them
        ctx.save_for_backward(out, module.time_enc.lin.weight, module.time_enc.lin.bias)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        module, s = ctx.module, ctx.s
        need = ctx.needs_input_grad
        params = param_list(module)
        grads: List[Optional[Tensor]] = [None] * (6 + len(params))
        out, tw, tb = ctx.saved_tensors
        aconv, phi = module.aconv, module.aconv.phi
        U, E, M, D, T, in_ch, dev = s.U, s.E, s.M, s.D, s.T, s.in_ch, out.device
        g = _rows(g)
        # id(parameter) -> (the group's tensor, index of its view in it)
        slots = {id(phi.lin_query.weight): ('W4', 0), id(phi.lin_key.weight): ('W4', 1), id(phi.lin_value.weight): ('W4', 2),
                 id(phi.lin_query.bias): ('b4', 0), id(phi.lin_key.bias): ('b4', 1), id(phi.lin_value.bias): ('b4', 2), id(aconv.bias): ('b4', 3),
                 id(aconv.W): ('W', None), id(module.enc_x.weight): ('Wx', None), id(module.enc_x.bias): ('bx', None),
                 id(phi.lin_edge.weight): ('We', None), id(module.time_enc.lin.weight): ('time', 0), id(module.time_enc.lin.bias): ('time', 1)}  # fmt: skip
        wanted = {slots[id(p)][0] for p, n in zip(params, need[6:]) if n}
        dW4, db4, dW, dWx, dbx, dx, dWe, dtime = _grad_views([(4, M, M), (4, M), (M, M), (M, in_ch), (M,), (U, in_ch), (M, D + T), (2, T)], dev)
        W4T, WxT, WeT = s.WT
        a = _native.CtanBwd()
        a.U, a.E, a.in_ch, a.M, a.D, a.T, a.num_iters = U, E, in_ch, M, D, T, s.num_iters
        a.epsilon, a.mean_delta_t, a.std_delta_t = float(aconv.epsilon), float(module.mean_delta_t), float(module.std_delta_t)
        a.g, a.ldg, a.out, a.x_save, a.node_x = g.data_ptr(), g.stride(0), out.data_ptr(), s.x_save.data_ptr(), s.node_x.data_ptr()
        a.last_update, a.t = s.last_update.data_ptr(), s.t.data_ptr()
        a.tw, a.tb = tw.detach().data_ptr(), tb.detach().data_ptr()
        a.W4, a.b4, a.W4T, a.WxT, a.WeT = s.W4.data_ptr(), s.b4.data_ptr(), W4T.data_ptr(), WxT.data_ptr(), WeT.data_ptr()
        f0, i0 = s.kept.data_ptr(), s.kept_i.data_ptr()
        a.edge_attr, a.eproj = f0, f0 + 4 * s.o_ep
        a.src_ok, a.order, a.seg_lo, a.seg_hi = i0, i0 + 8 * E, i0 + 16 * E, i0 + 8 * (2 * E + U)
        a.d_W4 = dW4.data_ptr() if wanted & {'W4', 'W'} else None
        a.d_b4 = db4.data_ptr() if 'b4' in wanted else None
        a.d_W = dW.data_ptr() if 'W' in wanted else None
        a.d_Wx = dWx.data_ptr() if 'Wx' in wanted else None
        a.d_bx = dbx.data_ptr() if 'bx' in wanted else None
        a.d_node_x = dx.data_ptr() if need[5] else None
        a.d_Wedge = dWe.data_ptr() if 'We' in wanted else None
        a.d_time = dtime.data_ptr() if 'time' in wanted else None
        _run(a, dev)
        grads[5] = dx if need[5] else None
        group = dict(W4=dW4, b4=db4, W=dW, Wx=dWx, bx=dbx, We=dWe)
        for i, (p, n) in enumerate(zip(params, need[6:])):
            if n:
                kind, ix = slots[id(p)]
                if kind == 'time':
                    grads[6 + i] = dtime[ix].view(p.shape)
                else:
                    grads[6 + i] = group[kind] if ix is None else group[kind][ix]
        return tuple(grads)


def apply(module, node_x: Tensor, last_update: Tensor, edge_index: Tensor, t: Tensor, msg: Tensor) -> Tensor:
    """The encoder's training path: ``out`` with ``grad_fn`` = :class:`CtanFunction`."""
    return CtanFunction.apply(module, last_update, edge_index, t, msg, node_x, *param_list(module))


# ---- the launches of tgmx_ctan_backward, one ctypes call each (TGMX_CTAN_BWD=py) ---------------------------------------------------------------
def backward_per_launch(a, dev) -> None:
    """What ``tgmx_ctan_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here."""
    lib, st = _native.load(), _native.stream_ptr()
    U, E, M, T, Wd, n_it, in_ch = a.U, a.E, a.M, a.T, a.D + a.T, a.num_iters, a.in_ch
    UM = U * M
    keep: list = []

    def buf(n: int, dtype=torch.float32) -> int:
        keep.append(torch.empty(max(1, n), dtype=dtype, device=dev))
        return keep[-1].data_ptr()

    def zero(p, n: int) -> None:  # (the native call clears with a memset; here a copy of zeros)
        if p:
            keep.append(torch.zeros(n, dtype=torch.float32, device=dev))
            _native.check(lib.tgmx_add_cols(p, n, keep[-1].data_ptr(), n, 1, n, 0, st), 'tgmx_add_cols')

    def tn_ws(R: int, m: int, n: int, batch: int) -> int:
        return buf(lib.tgmx_sgemm_tn_workspace_bytes(R, m, n, batch) // 4 + 1)

    walk = n_it > 0 and E > 0
    want_e = walk and bool(a.d_Wedge or a.d_time)
    want_x0 = bool(a.d_Wx or a.d_bx or a.d_node_x)
    gx, gx2, qkvs, d4 = buf(UM), buf(UM), buf(4 * UM), buf(4 * UM)
    alpha, sc, etgt = buf(E), buf(E), buf(E, torch.int32)
    order_s, sseg_lo, sseg_hi = buf(E, torch.int64), buf(U, torch.int64), buf(U, torch.int64)
    d_eproj = buf(E * M) if want_e else None
    cs_ws = buf(256 * max(4 * M, 2 * T))
    # 1. the final tanh
    _native.check(lib.tgmx_ctan_out_backward(a.g, a.ldg, a.out, U, M, gx, st), 'tgmx_ctan_out_backward')
    # 2. the iterations, last first
    if walk:
        nbytes = int(lib.tgmx_segment_sort_workspace_bytes(E))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.tgmx_segment_sort(a.src_ok, E, U, order_s, sseg_lo, sseg_hi, buf(nbytes, torch.uint8), nbytes, status.data_ptr(), st),
                      'tgmx_segment_sort')
    scale = float(np.float32(1.0) / np.sqrt(np.float32(M)))  # float32 arithmetic, as the C call computes it
    h4 = qkvs + 4 * 3 * UM
    for it in range(n_it - 1, -1, -1):
        x, first = a.x_save + 4 * it * UM, it == n_it - 1
        _native.check(lib.tgmx_sgemm_nt(x, M, a.W4, M, qkvs, M, U, M, M, a.b4, 0, 4, 0, M * M, UM, st), 'tgmx_sgemm_nt')
        _native.check(lib.tgmx_ctan_attend_backward(qkvs, qkvs + 4 * UM, qkvs + 8 * UM, h4, a.eproj, a.order, a.src_ok, a.seg_lo if E else None, a.seg_hi, U, M,
                                                    scale, a.epsilon, gx, d4, alpha, sc, etgt, d_eproj, 0 if first else 1, st), 'tgmx_ctan_attend_backward')  # fmt: skip
        _native.check(lib.tgmx_ctan_source_backward(qkvs, d4, order_s, etgt, sseg_lo if E else None, sseg_hi, alpha, sc, U, M, st), 'tgmx_ctan_source_backward')
        if a.d_W4:  # d_b^T x_it, batched over [q, k, v, z]
            _native.check(lib.tgmx_sgemm_tn(d4, 4 * M, x, M, a.d_W4, M, U, M, M, 4, M, 0, M * M, 0 if first else 1, tn_ws(U, M, M, 4), st), 'tgmx_sgemm_tn')
        if a.d_b4:
            _native.check(lib.tgmx_colsum(d4, 4 * M, U, 4 * M, a.d_b4, 0 if first else 1, cs_ws, st), 'tgmx_colsum')
        if it > 0 or want_x0:  # gx + d4 [W_q; W_k; W_v; A]
            _native.check(lib.tgmx_sgemm_nt_ep(d4, 4 * M, a.W4T, 4 * M, gx2, M, U, M, 4 * M, None, 0, gx, M, st), 'tgmx_sgemm_nt_ep')
            gx, gx2 = gx2, gx
    # 3. what lies around the loop
    if n_it == 0:
        zero(a.d_W4, 4 * M * M)
        zero(a.d_b4, 4 * M)
    if a.d_W:
        _native.check(lib.tgmx_ctan_antisym_grad(a.d_W4 + 4 * 3 * M * M, M, a.d_W, st), 'tgmx_ctan_antisym_grad')
    if a.d_Wx:
        _native.check(lib.tgmx_sgemm_tn(gx, M, a.node_x, in_ch, a.d_Wx, in_ch, U, M, in_ch, 1, 0, 0, 0, 0, tn_ws(U, M, in_ch, 1), st), 'tgmx_sgemm_tn')
    if a.d_bx:
        _native.check(lib.tgmx_colsum(gx, M, U, M, a.d_bx, 0, cs_ws, st), 'tgmx_colsum')
    if a.d_node_x:
        _native.check(lib.tgmx_sgemm_nt(gx, M, a.WxT, M, a.d_node_x, in_ch, U, in_ch, M, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')
    if not want_e:
        zero(a.d_Wedge, M * Wd)
        zero(a.d_time, 2 * T)
        return
    if a.d_Wedge:
        _native.check(lib.tgmx_sgemm_tn(d_eproj, M, a.edge_attr, Wd, a.d_Wedge, Wd, E, M, Wd, 1, 0, 0, 0, 0, tn_ws(E, M, Wd, 1), st), 'tgmx_sgemm_tn')
    if a.d_time:
        d_attr, part = buf(E * T), buf(E * 2 * T)
        _native.check(lib.tgmx_sgemm_nt(d_eproj, M, a.WeT, M, d_attr, T, E, T, M, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')
        _native.check(lib.tgmx_ctan_edge_attr_backward(a.last_update, a.src_ok, a.t, a.tw, a.tb, d_attr, T, T, E, a.mean_delta_t, a.std_delta_t, part, st),
                      'tgmx_ctan_edge_attr_backward')
        _native.check(lib.tgmx_colsum(part, 2 * T, E, 2 * T, a.d_time, 0, cs_ws, st), 'tgmx_colsum')


__all__ = ['CtanFunction', 'MAX_M', 'apply', 'backward_per_launch', 'in_envelope', 'mode', 'transposed_weights']
