"""Training path of ``NCNPredictor``: a ``torch.autograd.Function`` whose forward is ``tgmx_ncn_forward`` itself (so the result is the
no-grad call's, bit for bit) and whose backward is ONE native call (``tgmx_ncn_backward``, ``csrc/ncn_bwd.hip``):

    the last layer                 -> ``tgmx_decoder_tail_bwd`` (out <= 16 and the weight fits 48 KB; the ReLU mask is read from the saved h),
                                      else ``tgmx_sgemm_tn`` + ``tgmx_colsum`` + ``tgmx_sgemm_nt`` on a packed transpose + ``tgmx_relu_mask``
    the first layer                -> ``tgmx_sgemm_tn`` (dW1 = dpre^T xs), ``tgmx_colsum`` (db1)
    x (only when it wants one)     -> ``tgmx_sgemm_nt`` (dxs = dpre W1), then ``tgmx_ncn_dx``: node-centred, through two inverted indexes of
                                      the pairs and the adjacency the forward built, no float atomics

``TGMX_NCN_BWD=py`` issues the backward's launches one ctypes call each from :func:`backward_per_launch` -- the readable specification,
the same bits; ``TGMX_NCN_BWD=torch`` keeps the composed torch path (the module then never comes here).

What the backward reads -- ``xs``, ``h``, the last-occurrence marks and, without a prepared adjacency, ``indptr`` / ``cols`` -- lives in
buffers of the call: a training step calls the decoder for the positives and again for the negatives before one ``backward()``.  Only the
adjacency build's sort workspace, which nothing reads afterwards, stays in the module's scratch.  The weights are read where they are.
"""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _native
from ._fwd_plumbing import carve_scratch, up4
from ._paramver import param_list


def mode() -> str:
    """'native' (default), 'py' or 'torch': ``TGMX_NCN_BWD``."""
    m = os.environ.get('TGMX_NCN_BWD', '')
    return m if m in ('py', 'torch') else 'native'


def _up64(n: int) -> int:
    return (n + 63) // 64 * 64


def in_envelope(module, x: Tensor) -> bool:
    """The native training path takes the call: k = 2 / 4 (there is no native k = 8 backward), no autocast, contiguous float32 parameters on
    x's device."""
    if module.k == 8 or mode() == 'torch' or torch.is_autocast_enabled():
        return False
    return all(p.dtype == torch.float32 and p.is_contiguous() and p.device == x.device for p in param_list(module))


class NcnFunction(torch.autograd.Function):
    """``a``: the checked inputs of ``NCNPredictor._inputs`` (``x`` is ``a['x']``); the tensors after it: ``x``, ``xsmlp.0.weight``,
    ``xsmlp.0.bias``, ``xsmlp.2.weight``, ``xsmlp.2.bias``."""

    @staticmethod
    def forward(ctx, mod, a: dict, x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
        N, B, C, k, H, O = a['N'], a['B'], mod.in_channels, mod.k, mod.hidden_dim, mod.out_channels
        dev = x.device
        adj = a['adj']
        E = adj.num_edges if adj is not None else a['ei'].shape[1]
        ldxs, ldh = up4(k * C), up4(H)
        c = SimpleNamespace(a=a, adj=adj, N=N, B=B, E=E, weights=(w1, b1, w2, b2))
        # floats: xs, h;  int32: last [2 N], then (without a prepared adjacency) indptr [N + 1] and cols [2 E] -- all owned by this call
        sizes = [_up64(B * ldxs), _up64(B * ldh)]
        c.acts = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        xs, h = c.acts.split(sizes)
        isz = [_up64(2 * N), 0 if adj is not None else _up64(N + 1), 0 if adj is not None else _up64(max(2 * E, 1))]
        c.ints = torch.empty(sum(isz), dtype=torch.int32, device=dev)
        last, indptr, cols = c.ints.split(isz)
        c.out = torch.empty((B, O), dtype=torch.float32, device=dev)
        t = c.t = _native.NcnBwd()
        blk = t.fwd
        blk.w1, blk.b1, blk.w2, blk.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
        blk.C, blk.k, blk.H, blk.out_ch = C, k, H, O
        blk.x, blk.N = x.data_ptr(), N
        blk.decay, blk.dup_all = int(mod.cn_time_decay), int(mod.duplicate_targets == 'all')
        if adj is not None:
            blk.edge_index, blk.E, blk.have_adj = None, E, 1
            blk.indptr, blk.cols = adj.indptr.data_ptr(), adj.cols.data_ptr()
        else:
            from .ncn import _adj_ws_bytes

            need = _adj_ws_bytes(E)
            ws = carve_scratch(mod, [(need + 3) // 4], dev)[0]  # (the sort's workspace: nothing reads it after the build)
            blk.edge_index, blk.ei_stride, blk.E, blk.ei_is64, blk.have_adj = a['ei'].data_ptr(), a['ei_stride'], E, a['ei_is64'], 0
            blk.indptr, blk.cols = indptr.data_ptr(), cols.data_ptr()
            blk.adj_ws, blk.adj_ws_bytes = ws.data_ptr(), need
        tar = a['tar']
        blk.tar, blk.tar_stride, blk.B, blk.tar_is64 = tar.data_ptr(), max(B, 1), B, int(tar.dtype == torch.int64)
        blk.last_update, blk.edge_time = _native.ptr(a['lu']), _native.ptr(a['et'])
        blk.last = last.data_ptr()
        blk.xs, blk.h, blk.ldxs, blk.ldh = xs.data_ptr(), h.data_ptr(), ldxs, ldh
        blk.out = c.out.data_ptr()
        _native.check(_native.load().tgmx_ncn_forward(ctypes.byref(blk), _native.stream_ptr()), 'tgmx_ncn_forward')
        blk.adj_ws, blk.adj_ws_bytes = None, 0  # (the module's scratch: not the call's to keep)
        ctx.c = c
        return c.out.view(-1)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout: Tensor):
        c = ctx.c
        t = c.t
        blk = t.fwd
        x = c.a['x']
        dev = x.device
        O = blk.out_ch
        dout = dout.reshape(c.B, O).contiguous().float()
        need_x, *need_p = ctx.needs_input_grad[2:]
        sizes = [_up64(p.numel()) for p in c.weights]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        views = [v[: p.numel()].view(p.shape) for v, p in zip(flat.split(sizes), c.weights)]
        dx = torch.empty((c.N, blk.C), dtype=torch.float32, device=dev) if need_x else None
        t.dout, t.lddout = dout.data_ptr(), O
        t.d_x = _native.ptr(dx)
        t.d_w1, t.d_b1, t.d_w2, t.d_b2 = (v.data_ptr() if need else None for v, need in zip(views, need_p))
        if mode() == 'py':
            backward_per_launch(t, dev, [g for g in (dx, *(v for v, need in zip(views, need_p) if need)) if g is not None])
        else:
            lib = _native.load()
            need = int(lib.tgmx_ncn_backward_workspace_bytes(ctypes.byref(t)))
            if need == 0:
                _native.check(-1, 'tgmx_ncn_backward_workspace_bytes')
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            t.workspace, t.workspace_bytes = ws.data_ptr(), need
            _native.check(lib.tgmx_ncn_backward(ctypes.byref(t), _native.stream_ptr()), 'tgmx_ncn_backward')
            t.workspace, t.workspace_bytes = None, 0
        return (None, None, dx, *(v if need else None for v, need in zip(views, need_p)))


def apply(mod, a: dict) -> Tensor:
    """``NCNPredictor.forward`` under gradients: [B * out_channels]."""
    m = mod.xsmlp
    return NcnFunction.apply(mod, a, a['x'], m[0].weight, m[0].bias, m[2].weight, m[2].bias)


# ---- the launches of tgmx_ncn_backward, one ctypes call each (TGMX_NCN_BWD=py) -----------------------------------------------------------------
def _tail_route(out_ch: int, H: int) -> bool:
    return out_ch <= _native.DECODER_MAX_TAIL and out_ch * H * 4 <= 48 * 1024


def backward_per_launch(t, dev, grads=()) -> None:
    """What ``tgmx_ncn_backward`` composes, in its order with its kernels; every buffer of the native call's workspace is a tensor here
    (``grads``: the tensors behind the block's gradient pointers)."""
    lib, st = _native.load(), _native.stream_ptr()
    a = t.fwd
    B, H, O, K = a.B, a.H, a.out_ch, a.k * a.C
    keep: list = []

    def buf(n: int, dtype=torch.float32) -> int:
        keep.append(torch.empty(max(1, n), dtype=dtype, device=dev))
        return keep[-1].data_ptr()

    if B == 0:  # no pair: the native call clears the gradients asked for (memsets, no launch)
        for g in grads:
            g.zero_()
        return

    def tn(A, lda, Bm, ldb, C, ldc, M, N):
        part = buf(lib.tgmx_sgemm_tn_workspace_bytes(B, M, N, 1) // 4)
        _native.check(lib.tgmx_sgemm_tn(A, lda, Bm, ldb, C, ldc, B, M, N, 1, 0, 0, 0, 0, part, st), 'tgmx_sgemm_tn')

    def colsum(X, ld, C, out):
        _native.check(lib.tgmx_colsum(X, ld, B, C, out, 0, buf(256 * C), st), 'tgmx_colsum')

    def nt(A, lda, Bm, ldb, C, ldc, N, Kk):
        _native.check(lib.tgmx_sgemm_nt(A, lda, Bm, ldb, C, ldc, B, N, Kk, None, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')

    want_dpre = bool(t.d_x) or bool(t.d_w1) or bool(t.d_b1)
    tail = _tail_route(O, H)
    dpre = buf(B * H) if want_dpre else None
    dxs = buf(B * K) if t.d_x else None
    packs = []
    w2t = w1t = None
    if want_dpre and not tail:
        w2t = buf(H * O)
        packs.append((a.w2, w2t, H, O))
    if t.d_x:
        w1t = buf(K * H)
        packs.append((a.w1, w1t, K, H))
    if packs:
        jobs = (_native.PackJob * len(packs))()
        for j, (src, dst, r, c_) in zip(jobs, packs):  # src [c_, r] -> dst [r, c_]
            j.src, j.dst, j.src_ld, j.dst_ld, j.rows, j.cols, j.dst_rows, j.dst_cols, j.transpose = src, dst, r, c_, r, c_, r, c_, 1
        _native.check(lib.tgmx_pack2d(jobs, len(packs), st), 'tgmx_pack2d')
    if tail:
        floats = lib.tgmx_decoder_tail_bwd_workspace_floats(B, H, O) if (t.d_w2 or t.d_b2) else 0
        _native.check(lib.tgmx_decoder_tail_bwd(t.dout, t.lddout, a.h, a.ldh, B, H, a.w2, O, 1, dpre, H, t.d_w2, t.d_b2, buf(floats), floats, st),
                      'tgmx_decoder_tail_bwd')  # fmt: skip
    else:
        if t.d_w2:
            tn(t.dout, t.lddout, a.h, a.ldh, t.d_w2, H, O, H)
        if t.d_b2:
            colsum(t.dout, t.lddout, O, t.d_b2)
        if want_dpre:
            nt(t.dout, t.lddout, w2t, O, dpre, H, H, O)
            _native.check(lib.tgmx_relu_mask(dpre, H, a.h, a.ldh, B, H, st), 'tgmx_relu_mask')
    if t.d_w1:
        tn(dpre, H, a.xs, a.ldxs, t.d_w1, K, H, K)
    if t.d_b1:
        colsum(dpre, H, H, t.d_b1)
    if t.d_x:
        nt(dpre, H, w1t, H, dxs, K, K, H)
        nbytes = int(lib.tgmx_ncn_dx_workspace_bytes(a.N, a.E, B, a.C))
        _native.check(lib.tgmx_ncn_dx(a.x, a.N, a.C, a.k, a.indptr, a.cols, a.E, a.tar, a.tar_is64, a.tar_stride, B, a.last_update if a.decay else None,
                                      a.edge_time if a.decay else None, None if a.dup_all else a.last, dxs, K, t.d_x, buf(nbytes, torch.uint8), nbytes,
                                      st), 'tgmx_ncn_dx')  # fmt: skip


__all__ = ['NcnFunction', 'apply', 'backward_per_launch', 'in_envelope', 'mode']
