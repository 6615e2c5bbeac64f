"""Training path of the TGN modules: ``torch.autograd.Function``s whose forwards are the same native kernels as
inference and whose backwards are hand-written (``csrc/tgn_bwd.hip``) or composed from the GEMM blocks of the TGAT
backward (``tgmx_sgemm_nt`` with transposed weights for dX, ``tgmx_sgemm_tn`` for dW, ``tgmx_colsum`` for biases and
the Time2Vec parameters).  The reference trains through torch autograd (``examples/linkproppred/tgn.py:97-118``);
``memory`` / ``last_update`` are buffers, so gradients reach the shared Time2Vec, the GRU cell and the TransformerConv
projections (and flow back through ``x``, the memory module's output).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from .. import _native
from . import _ops


def native_backward_selected() -> bool:
    """``TGMX_TGN_BWD=native``: the one-call layer backward / the deterministic attention kernels for heads of up to 64 channels too
    (wider heads always take them).  Read per call: the tests switch it."""
    return os.environ.get('TGMX_TGN_BWD', '') == 'native'


def train_supported(H: int, C: int) -> bool:
    """The envelope of csrc/tconv_bwd.hip, asked of the library itself: C <= 256, H <= 8, H C <= 512."""
    return bool(_native.load().tgmx_tconv_train_supported(H, C))


def _colsum(X: Tensor, R: int, C: int) -> Tensor:
    lib = _native.load()
    out = torch.empty(C, dtype=torch.float32, device=X.device)
    ws = torch.empty(256 * C, dtype=torch.float32, device=X.device)
    _native.check(lib.tgmx_colsum(X.data_ptr(), X.stride(0), R, C, out.data_ptr(), 0, ws.data_ptr(), _native.stream_ptr()), 'tgmx_colsum')
    return out


def _sgemm_tn(A: Tensor, B: Tensor) -> Tensor:
    """A^T B: A [R, M], B [R, N] -> [M, N] (weight gradient: reduction over the rows)."""
    lib = _native.load()
    R, M, N = A.shape[0], A.shape[1], B.shape[1]
    C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    need = int(lib.tgmx_sgemm_tn_workspace_bytes(R, M, N, 1))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=A.device)
    _native.check(lib.tgmx_sgemm_tn(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), R, M, N, 1, 0, 0, 0, 0,
                                    ws.data_ptr(), _native.stream_ptr()), 'tgmx_sgemm_tn')  # fmt: skip
    return C


class LinearFn(torch.autograd.Function):
    """y = x W^T (+ b) on the native GEMM."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
        x = x.contiguous()
        y = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.float32, device=x.device)
        if x.shape[0]:
            _ops.sgemm_nt(x, weight.detach().contiguous(), y, bias=None if bias is None else bias.detach())
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        R = x.shape[0]
        dx = dw = db = None
        if R == 0:
            return (torch.zeros_like(x) if ctx.needs_input_grad[0] else None, torch.zeros_like(weight),
                    torch.zeros(weight.shape[0], device=x.device) if ctx.has_bias else None)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _ops.sgemm_nt(dy, weight.detach().t().contiguous(), dx)  # dx = dy W
        if ctx.needs_input_grad[1]:
            dw = _sgemm_tn(dy, x)  # dW = dy^T x
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _colsum(dy, R, dy.shape[1])
        return dx, dw, db


class GruGateFn(torch.autograd.Function):
    """out = GRUCell gate arithmetic on precomputed gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh (h: buffer rows)."""

    @staticmethod
    def forward(ctx, gi: Tensor, gh: Tensor, h: Tensor) -> Tensor:
        lib = _native.load()
        R, M = h.shape
        out = torch.empty((R, M), dtype=torch.float32, device=h.device)
        _native.check(lib.tgmx_tgn_gru_gate(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), M, R, out.data_ptr(), _native.stream_ptr()), 'tgmx_tgn_gru_gate')
        ctx.save_for_backward(gi, gh, h)
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        gi, gh, h = ctx.saved_tensors
        lib = _native.load()
        R, M = h.shape
        dgi, dgh = torch.empty_like(gi), torch.empty_like(gh)
        _native.check(lib.tgmx_tgn_gru_gate_backward(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), dout.contiguous().data_ptr(), M, R,
                                                     dgi.data_ptr(), dgh.data_ptr(), _native.stream_ptr()), 'tgmx_tgn_gru_gate_backward')  # fmt: skip
        return dgi, dgh, None


class AggregateFn(torch.autograd.Function):
    """aggr rows of TGNMemory (tgmx_tgn_aggregate); differentiable w.r.t. the Time2Vec weight / bias."""

    @staticmethod
    def forward(ctx, tw: Tensor, tb: Tensor, mem_module, nodes: Tensor, assoc=None, stamp: int = 0):
        m = mem_module
        lib = _native.load()
        dev, R, M, D, T = nodes.device, nodes.numel(), m.memory_dim, m.raw_msg_dim, m.time_dim
        W = 2 * M + D + T
        aggr = torch.empty((R, W), dtype=torch.float32, device=dev)
        new_lu = torch.empty(R, dtype=torch.int64, device=dev)
        twc, tbc = tw.detach().reshape(-1).contiguous(), tb.detach().contiguous()
        _native.check(
            lib.tgmx_tgn_aggregate(
                nodes.data_ptr(), R, m.memory.data_ptr(), m.last_update.data_ptr(), M, m.num_nodes, m._st_lo[0].data_ptr(),
                m._st_cnt[0].data_ptr(), m._st_lo[1].data_ptr(), m._st_cnt[1].data_ptr(), _native.ptr(m._log_other), _native.ptr(m._log_t),
                _native.ptr(m._log_raw), D, twc.data_ptr(), tbc.data_ptr(), T, m.aggr_module.mean, aggr.data_ptr(), new_lu.data_ptr(),
                _native.ptr(assoc), stamp, _native.stream_ptr(),
            ),
            'tgmx_tgn_aggregate',
        )  # fmt: skip
        # the reference's training loop calls update_state BEFORE loss.backward(): snapshot the rows' message windows and
        # last_update now (the event log itself is append-only within an epoch; ctx keeps this log tensor alive)
        idx = nodes.long()
        idx = torch.where(idx < 0, idx + m.num_nodes, idx)
        ctx.rows = (m._st_lo[0][idx], m._st_cnt[0][idx], m._st_lo[1][idx], m._st_cnt[1][idx], m.last_update[idx], m._log_t)
        ctx.dims = (R, M, D, T, m.aggr_module.mean)
        ctx.twc, ctx.tbc, ctx.tw_shape = twc, tbc, tw.shape
        ctx.mark_non_differentiable(new_lu)
        return aggr, new_lu

    @staticmethod
    def backward(ctx, d_aggr: Tensor, _d_lu):
        lo0, c0, lo1, c1, lu, log_t = ctx.rows
        R, M, D, T, mean = ctx.dims
        lib = _native.load()
        dev = ctx.twc.device
        if R == 0:
            return torch.zeros(ctx.tw_shape, device=dev), torch.zeros(T, device=dev), None, None, None, None
        part = torch.empty((R, 2 * T), dtype=torch.float32, device=dev)
        _native.check(
            lib.tgmx_tgn_aggregate_backward(R, lo0.data_ptr(), c0.data_ptr(), lo1.data_ptr(), c1.data_ptr(), lu.data_ptr(), _native.ptr(log_t),
                                            M, D, ctx.twc.data_ptr(), ctx.tbc.data_ptr(), T, mean, d_aggr.contiguous().data_ptr(),
                                            part.data_ptr(), _native.stream_ptr()),
            'tgmx_tgn_aggregate_backward',
        )  # fmt: skip
        g = _colsum(part, R, 2 * T)
        return g[:T].reshape(ctx.tw_shape), g[T:], None, None, None, None


class EdgeAttrFn(torch.autograd.Function):
    """edge_attr = [Time2Vec(last_update[src] - t) | msg] (tgmx_tconv_edge_attr); differentiable w.r.t. Time2Vec."""

    @staticmethod
    def forward(ctx, tw: Tensor, tb: Tensor, lu_local: Tensor, src: Tensor, t: Tensor, msg: Tensor) -> Tensor:
        lib = _native.load()
        E, T, D = src.numel(), tb.numel(), msg.shape[1]
        out = torch.empty((E, T + D), dtype=torch.float32, device=msg.device)
        twc, tbc = tw.detach().reshape(-1).contiguous(), tb.detach().contiguous()
        _native.check(lib.tgmx_tconv_edge_attr(lu_local.data_ptr(), src.data_ptr(), t.data_ptr(), msg.data_ptr(), twc.data_ptr(), tbc.data_ptr(),
                                               T, D, E, out.data_ptr(), _native.stream_ptr()), 'tgmx_tconv_edge_attr')  # fmt: skip
        ctx.saved = (lu_local, src, t, twc, tbc, T, D, E, tw.shape)
        return out

    @staticmethod
    def backward(ctx, d_attr: Tensor):
        lu_local, src, t, twc, tbc, T, D, E, tw_shape = ctx.saved
        lib = _native.load()
        if E == 0:
            return torch.zeros(tw_shape, device=twc.device), torch.zeros(T, device=twc.device), None, None, None, None
        part = torch.empty((E, 2 * T), dtype=torch.float32, device=twc.device)
        _native.check(lib.tgmx_tconv_edge_attr_backward(lu_local.data_ptr(), src.data_ptr(), t.data_ptr(), twc.data_ptr(), tbc.data_ptr(),
                                                        d_attr.contiguous().data_ptr(), T, D, E, part.data_ptr(), _native.stream_ptr()),
                      'tgmx_tconv_edge_attr_backward')  # fmt: skip
        g = _colsum(part, E, 2 * T)
        return g[:T].reshape(tw_shape), g[T:], None, None, None, None


class TconvAttendFn(torch.autograd.Function):
    """out = skip + per-target softmax attention (tgmx_tconv_attend)."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, eproj: Tensor, skip: Tensor, order: Tensor, src: Tensor, seg_lo: Tensor,
                seg_hi: Tensor, H: int, C: int, drop: tuple = (0.0, 0, 0)) -> Tensor:  # fmt: skip
        lib = _native.load()
        out = skip.clone()
        U = q.shape[0]
        _native.check(lib.tgmx_tconv_attend(q.data_ptr(), k.data_ptr(), v.data_ptr(), eproj.data_ptr(), order.data_ptr(), src.data_ptr(),
                                            seg_lo.data_ptr(), seg_hi.data_ptr(), U, H, C, float(C) ** -0.5, out.data_ptr(),
                                            _native.dropout_desc(*drop), _native.stream_ptr()),
                      'tgmx_tconv_attend')  # fmt: skip
        ctx.save_for_backward(q, k, v, eproj, order, src, seg_lo, seg_hi)
        ctx.H, ctx.C, ctx.drop = H, C, drop
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        q, k, v, eproj, order, src, seg_lo, seg_hi = ctx.saved_tensors
        lib = _native.load()
        dout = dout.contiguous()
        dq = torch.empty_like(q)
        de = torch.empty_like(eproj)
        if ctx.C > 64 or native_backward_selected():
            # the deterministic kernels (csrc/tconv_bwd.hip): every element written once, no zero-initialisation
            U, E = q.shape[0], eproj.shape[0]
            dk, dv = torch.empty_like(k), torch.empty_like(v)
            ws = torch.empty(max(int(lib.tgmx_tconv_attend_backward_det_workspace_bytes(U, E, ctx.H)), 4), dtype=torch.uint8, device=q.device)
            _native.check(lib.tgmx_tconv_attend_backward_det(q.data_ptr(), k.data_ptr(), v.data_ptr(), eproj.data_ptr(), order.data_ptr(), src.data_ptr(),
                                                             seg_lo.data_ptr(), seg_hi.data_ptr(), U, E, ctx.H, ctx.C, float(ctx.C) ** -0.5,
                                                             dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), de.data_ptr(),
                                                             _native.dropout_desc(*ctx.drop), ws.data_ptr(), ws.numel(), _native.stream_ptr()),
                          'tgmx_tconv_attend_backward_det')  # fmt: skip
            return dq, dk, dv, de, dout, None, None, None, None, None, None, None
        dk, dv = torch.zeros_like(k), torch.zeros_like(v)
        _native.check(lib.tgmx_tconv_attend_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), eproj.data_ptr(), order.data_ptr(), src.data_ptr(),
                                                     seg_lo.data_ptr(), seg_hi.data_ptr(), q.shape[0], ctx.H, ctx.C, float(ctx.C) ** -0.5,
                                                     dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), de.data_ptr(),
                                                     _native.dropout_desc(*ctx.drop), _native.stream_ptr()), 'tgmx_tconv_attend_backward')  # fmt: skip
        return dq, dk, dv, de, dout, None, None, None, None, None, None, None


class TconvLayerFn(torch.autograd.Function):
    """GraphAttentionEmbedding's layer as ONE node: z = TransformerConv(x, [Time2Vec(last_update[src] - t) | msg]).  The forward is the
    inference call with the dropout descriptor passed through (``tgmx_tconv_forward_train``), the backward one native call
    (``tgmx_tconv_backward``).  Everything the backward reads is kept here at forward time: the reference's training loop calls
    ``memory.update_state`` before ``loss.backward()``."""

    @staticmethod
    def forward(ctx, x, tw, tb, wq, bq, wk, bk, wv, bv, we, ws_, bs, conv, lu: Tensor, edge_index: Tensor, t: Tensor, msg: Tensor, drop: tuple):
        lib = _native.load()
        dev, U, H, C = x.device, x.shape[0], conv.heads, conv.out_channels
        HC, E, T, D = H * C, edge_index.shape[1], tb.numel(), msg.shape[1]
        f32 = dict(dtype=torch.float32, device=dev)
        x = _ops._f32c(x.detach(), 'x')
        W4, b4 = conv._stacked_projections()
        we = we.detach().contiguous()
        twc, tbc = tw.detach().reshape(-1).contiguous(), tb.detach().contiguous()
        src, tgt = edge_index[0].contiguous(), edge_index[1].contiguous()
        qkvs = torch.empty((4, U, HC), **f32)
        fl = torch.empty(E * (T + D + HC), **f32)  # edge_attr [E, T + D] | eproj [E, HC]
        Ep, Up = E + (E & 1), U + (U & 1)
        ints = torch.empty(2 * Ep + 3 * Up, dtype=torch.int64, device=dev)  # order | seg_lo | seg_hi | cursor | order_big
        need = int(lib.tgmx_segment_sort_workspace_bytes(E))
        wsd = getattr(conv, '_seg_ws', None)
        if wsd is None or wsd[0].device != dev or wsd[0].numel() < need:
            wsd = conv._seg_ws = (torch.empty(need, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        cnt = getattr(conv, '_tgt_count', None)
        if cnt is None or cnt.device != dev or cnt.numel() < U:
            cnt = conv._tgt_count = torch.zeros(max(2 * U, 1 << 14), dtype=torch.int32, device=dev)
        a = _native.TconvFwd()
        a.x, a.U, a.in_ch, a.last_update_local = x.data_ptr(), U, x.shape[1], lu.data_ptr()
        a.src, a.tgt, a.t, a.msg, a.E, a.D, a.T = src.data_ptr(), tgt.data_ptr(), t.data_ptr(), msg.data_ptr(), E, D, T
        a.tw, a.tb, a.W4, a.b4, a.W_edge, a.H, a.C = twc.data_ptr(), tbc.data_ptr(), W4.data_ptr(), b4.data_ptr(), we.data_ptr(), H, C
        a.edge_attr, a.qkvs, a.eproj = fl.data_ptr(), qkvs.data_ptr(), fl.data_ptr() + 4 * E * (T + D)
        a.order, a.seg_lo, a.seg_hi = ints.data_ptr(), ints.data_ptr() + 8 * Ep, ints.data_ptr() + 8 * (Ep + Up)
        a.sort_ws, a.sort_ws_bytes, a.status = wsd[0].data_ptr(), wsd[0].numel(), wsd[1].data_ptr()
        a.tgt_count, a.cursor, a.order_big = cnt.data_ptr(), ints.data_ptr() + 8 * (Ep + 2 * Up), ints.data_ptr() + 8 * (Ep + 3 * Up)
        _native.check(lib.tgmx_tconv_forward_train(a, _native.dropout_desc(*drop), _native.stream_ptr()), 'tgmx_tconv_forward_train')
        ctx.kept = (x, qkvs, fl, src, tgt, t, lu, twc, tbc, W4, we)
        ctx.dims = (U, E, H, C, T, D, tw.shape, drop)
        return qkvs[3]

    @staticmethod
    def backward(ctx, g: Tensor):
        x, qkvs, fl, src, tgt, t, lu, twc, tbc, W4, we = ctx.kept
        U, E, H, C, T, D, tw_shape, drop = ctx.dims
        lib = _native.load()
        HC, in_ch, dev = H * C, x.shape[1], x.device
        f32 = dict(dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        g = g.contiguous()
        a = _native.TconvBwd()
        a.U, a.E, a.in_ch, a.H, a.C, a.D, a.T = U, E, in_ch, H, C, D, T
        a.g, a.ldg, a.x, a.qkvs = g.data_ptr(), HC, x.data_ptr(), qkvs.data_ptr()
        a.edge_attr, a.eproj = fl.data_ptr(), fl.data_ptr() + 4 * E * (T + D)
        a.src, a.tgt, a.t, a.last_update_local, a.tw, a.tb = src.data_ptr(), tgt.data_ptr(), t.data_ptr(), lu.data_ptr(), twc.data_ptr(), tbc.data_ptr()
        if drop[0]:
            a.drop = _native.Dropout(float(drop[0]), drop[1] & 0xFFFFFFFFFFFFFFFF, drop[2] & 0xFFFFFFFFFFFFFFFF, 0)
        d_x = d_W4 = d_b4 = d_We = d_time = W4T = WeT = None
        if need[0]:
            d_x = torch.empty((U, in_ch), **f32)
            W4T = W4.reshape(4 * HC, in_ch).t().contiguous()
            a.d_x, a.W4T = d_x.data_ptr(), W4T.data_ptr()
        if any(need[i] for i in (3, 5, 7, 10)):
            d_W4 = torch.empty((4, HC, in_ch), **f32)
            a.d_W4 = d_W4.data_ptr()
        if any(need[i] for i in (4, 6, 8, 11)):
            d_b4 = torch.empty((4, HC), **f32)
            a.d_b4 = d_b4.data_ptr()
        if need[9]:
            d_We = torch.empty((HC, T + D), **f32)
            a.d_Wedge = d_We.data_ptr()
        if need[1] or need[2]:
            d_time = torch.empty(2 * T, **f32)
            WeT = we[:, :T].t().contiguous()
            a.d_time, a.WeT = d_time.data_ptr(), WeT.data_ptr()
        ws = torch.empty(max(int(lib.tgmx_tconv_backward_workspace_bytes(a)), 4), dtype=torch.uint8, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        _native.check(lib.tgmx_tconv_backward(a, _native.stream_ptr()), 'tgmx_tconv_backward')
        pick = lambda want, buf, i: buf[i] if (want and buf is not None) else None
        return (d_x, d_time[:T].reshape(tw_shape) if need[1] else None, d_time[T:] if need[2] else None,
                pick(need[3], d_W4, 0), pick(need[4], d_b4, 0), pick(need[5], d_W4, 1), pick(need[6], d_b4, 1),
                pick(need[7], d_W4, 2), pick(need[8], d_b4, 2), d_We, pick(need[10], d_W4, 3), pick(need[11], d_b4, 3),
                None, None, None, None, None, None)
