"""What the three decoders share: the MLP (``self.model``: Linear, ReLU, ..., Linear), the decision between the native head and torch ops,
the argument block of ``tgmx_decoder_forward`` cached against the parameters' versions, and the same launches issued one by one."""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace
from typing import List, Optional

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from . import _decoder_train
from ._fwd_plumbing import Unsupported, cached_block, carve_scratch, check_supported, needs_torch
from ._paramver import TransientCaches
from .aggregation import ConcatMerge, LearnableSumMerge
from ._snapshot import _Skipped

ACT_NONE, ACT_RELU = 0, 1


def build_mlp(in_dim: int, hidden_dim: int, out_dim: int, nlayers: int) -> nn.Sequential:
    """Linear(in, hidden), ReLU, [Linear(hidden, hidden), ReLU] x (nlayers - 2), Linear(hidden, out): nlayers = 1 gives the two of nlayers = 2."""
    mods: List[nn.Module] = [nn.Linear(in_dim, hidden_dim), nn.ReLU()]
    for _ in range(1, nlayers - 1):
        mods += [nn.Linear(hidden_dim, hidden_dim), nn.ReLU()]
    mods.append(nn.Linear(hidden_dim, out_dim))
    return nn.Sequential(*mods)


def linears(model: nn.Module) -> Optional[List[nn.Linear]]:
    """The Linears of a Linear / ReLU chain as the constructors build it; None for anything else (it then runs as torch ops)."""
    if not isinstance(model, nn.Sequential) or len(model) % 2 == 0:
        return None
    mods = list(model)
    if any(type(m) is not (nn.ReLU if i % 2 else nn.Linear) for i, m in enumerate(mods)):
        return None
    lins = mods[0::2]
    if len(lins) > _native.DECODER_MAX_LAYERS + 1 or any(a.out_features != b.in_features for a, b in zip(lins, lins[1:])):
        return None
    return lins


def _plain(t: Optional[Tensor], device) -> bool:
    return t is None or (t.device == device and t.dtype == torch.float32 and t.is_contiguous())


class DecoderHead(_Skipped, TransientCaches):
    """Mixin in front of ``nn.Module``: ``self.model`` runs natively through :meth:`_run`; ``check()`` reports indices outside the table."""

    def check(self) -> None:
        """Raise if a call saw an index outside ``[0, N')`` (the scores of such pairs are NaN).  Reads the device."""
        c = self.__dict__.get('_tgmx_skipped')
        if c is not None and int(c.item()):
            c.zero_()
            raise ValueError(f'{type(self).__name__}: an index pointed outside the embedding table; the scores of those pairs are NaN')

    def _native_ok(self, *inputs: Tensor) -> bool:
        x = inputs[0]
        if x.device.type != 'cuda' or any(t.device != x.device or t.dtype != torch.float32 for t in inputs):
            return False
        if needs_torch(self, 0.0, *inputs):
            return False
        lins = linears(self.model)
        return lins is not None and all(_plain(p, x.device) for p in self.parameters())

    def _trainable(self, *inputs: Tensor) -> bool:
        """The native training path applies (``_decoder_train.py``): autograd has something to track and the call is otherwise inside the
        native envelope -- on the device, float32 everywhere and no autocast, contiguous parameters, the constructor's layer chain, at
        least one row.  ``TGMX_DECODER_BWD=torch`` keeps the composed path."""
        x = inputs[0]
        if x.device.type != 'cuda' or any(t.device != x.device or t.dtype != torch.float32 for t in inputs) or x.shape[0] == 0:
            return False
        if not needs_torch(self, 0.0, *inputs) or torch.is_autocast_enabled() or _decoder_train.mode() == 'torch':
            return False
        lins = linears(self.model)
        return lins is not None and len(lins) - (self._merge_kind() == 'concat') <= _native.DECODER_MAX_LAYERS and all(
            _plain(p, x.device) for p in self.parameters())  # fmt: skip

    def _train(self, form: str, idx, shape: tuple, *inputs: Tensor) -> Tensor:
        return _decoder_train.apply(self, linears(self.model), self._merge_kind(), form, idx, shape, *inputs)

    def _merge_kind(self) -> Optional[str]:
        """'concat' / 'sum' when the merge is one of the two shipped and fits the model; None: the merge runs as torch ops."""
        m, lins = getattr(self, 'merge', None), linears(self.model)
        if lins is None:
            return None
        if type(m) is ConcatMerge and 2 * m.dim == lins[0].in_features and len(lins) >= 2:
            return 'concat'
        if type(m) is LearnableSumMerge and m.dim == lins[0].in_features and len(lins) <= _native.DECODER_MAX_LAYERS:
            return 'sum'
        return None

    # ---- the cached argument block --------------------------------------------------------------------------------------------------------
    def _weights(self, f32):
        """Every weight pointer of the head: the layers after the merge stage, the merge stage's operands for the pair form (slices of the
        parameters themselves) and for the table form (the stacked [Wa ; Wb] and [bias | 0])."""
        lins = linears(self.model)
        kind = self._merge_kind()
        w = SimpleNamespace(blk=_native.DecoderFwd(), kind=kind, pair=None, table=None, D=0, H=0, act=ACT_NONE)
        if kind == 'concat':
            first, rest = lins[0], lins[1:]
            D, H = self.merge.dim, first.out_features
            W0 = first.weight.detach()
            b0 = None if first.bias is None else first.bias.detach()
            p0 = f32(W0)
            w.pair = (p0, 2 * D, p0 + 4 * D, 2 * D, None if b0 is None else f32(b0, 'bias'))
            zeros = torch.zeros(H, dtype=torch.float32, device=W0.device)
            w.table = (f32(torch.cat((W0[:, :D], W0[:, D:]), dim=0)), D, f32(torch.cat((zeros if b0 is None else b0, zeros)), 'bias'))
            w.D, w.H, w.act = D, H, ACT_RELU
        elif kind == 'sum':
            rest = lins
            D = H = self.merge.dim
            Ws, Wd = self.merge.lin_src.weight.detach(), self.merge.lin_dst.weight.detach()
            bias = torch.zeros(D, dtype=torch.float32, device=Ws.device)
            for lin in (self.merge.lin_src, self.merge.lin_dst):
                if lin.bias is not None:
                    bias = bias + lin.bias.detach()
            w.pair = (f32(Ws), D, f32(Wd), D, f32(bias, 'bias'))
            w.table = (f32(torch.cat((Ws, Wd), dim=0)), D, f32(torch.cat((bias, torch.zeros_like(bias))), 'bias'))
            w.D, w.H, w.act = D, H, ACT_NONE
        else:
            rest = lins
            w.D = lins[0].in_features
        blk = w.blk
        blk.num_layers = len(rest)
        for ly, lin in zip(blk.layers, rest):
            ly.w, ly.b = f32(lin.weight), (None if lin.bias is None else f32(lin.bias, 'bias'))
            ly.in_, ly.out = lin.in_features, lin.out_features
        w.out_dim = rest[-1].out_features
        w.widest = max([w.H] + [lin.out_features for lin in rest[:-1]])
        return w

    def _run(self, form: str, R: int, fill, device, pool: Optional[str] = None, scratch=(0, 0, 0)) -> Tensor:
        """One head: ``fill(blk, w)`` sets the operands; returns out [R, out_dim].  ``scratch``: floats of P, the pooled row, the pool's
        chunk sums."""
        lib = _native.load()
        w, _keep = cached_block(self, self._weights)
        a = w.blk
        out = torch.empty((R, w.out_dim), dtype=torch.float32, device=device)
        if R == 0:
            return out
        a.form, a.pool, a.merge_act, a.D, a.H, a.R = _native.DECODER_FORM[form], _native.DECODER_POOL[pool], w.act, w.D, w.H, R
        a.a2 = a.ia = a.ib = a.neg = a.off = a.wa = a.wb = a.mbias = a.P = a.pooled = a.pool_ws = None
        a.idx64, a.M, a.max_candidates, a.B, a.pool_ws_floats = 0, -1, 0, 0, 0
        if form == 'pair':
            a.wa, a.ldwa, a.wb, a.ldwb, a.mbias = w.pair
        elif form == 'table':
            a.wa, a.ldwa, a.mbias = w.table
        bufs = carve_scratch(self, [R * w.widest, R * w.widest, *scratch], device)
        a.h[0], a.h[1] = bufs[0].data_ptr(), bufs[1].data_ptr()
        if scratch[0]:
            a.P = bufs[2].data_ptr()
        if scratch[1]:
            a.pooled = bufs[3].data_ptr()
        if scratch[2]:
            a.pool_ws, a.pool_ws_floats = bufs[4].data_ptr(), scratch[2]
        a.bad, a.out = self._skipped(device).data_ptr(), out.data_ptr()
        hold = fill(a, w)  # noqa: F841  (the tensors behind the operand pointers, alive until the call is issued)
        if os.environ.get('TGMX_DECODER_PY') == '1':
            forward_per_launch(a)
        else:
            check_supported(lib.tgmx_decoder_forward(ctypes.byref(a), _native.stream_ptr()), 'tgmx_decoder_forward')
        return out

    def _mlp_rows(self, x: Tensor) -> Tensor:
        """``self.model`` over the rows of x [R, in] (contiguous float32 on the device)."""

        def fill(a, w):
            a.a1, a.lda1, a.n1 = x.data_ptr(), x.stride(0), x.shape[0]
            return x

        return self._run('rows', x.shape[0], fill, x.device)


# ---- the launches of tgmx_decoder_forward, one ctypes call each (TGMX_DECODER_PY=1) ---------------------------------------------------------
def _layers(lib, a, x: int, ldx: int, R: int, st) -> None:
    flip = 0
    if R == 1 and all(max(a.layers[l].in_, a.layers[l].out) <= _native.DECODER_ROW_MLP_MAX for l in range(a.num_layers)):
        _native.check(lib.tgmx_decoder_row_mlp(x, a.layers, a.num_layers, a.out, st), 'tgmx_decoder_row_mlp')
        return
    for l in range(a.num_layers):
        ly = a.layers[l]
        last = l == a.num_layers - 1
        if last and ly.out <= _native.DECODER_MAX_TAIL and ly.out * ly.in_ * 4 <= 48 * 1024:
            _native.check(lib.tgmx_decoder_tail(x, ldx, R, ly.in_, ly.w, ly.b, ly.out, a.out, st), 'tgmx_decoder_tail')
            return
        y = a.out if last else a.h[flip]
        _native.check(lib.tgmx_sgemm_nt(x, ldx, ly.w, ly.in_, y, ly.out, R, ly.out, ly.in_, ly.b, 0 if last else 1, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')
        x, ldx, flip = y, ly.out, flip ^ 1


def forward_per_launch(a) -> None:
    lib, st = _native.load(), _native.stream_ptr()
    D, H = a.D, a.H
    if a.form == _native.DECODER_FORM['rows']:
        x, ldx, R = a.a1, a.lda1, a.R
        if a.pool:
            _native.check(lib.tgmx_pool_rows(x, ldx, a.n1, D, 1 if a.pool == _native.DECODER_POOL['mean'] else 0, a.pool_ws, a.pool_ws_floats, a.pooled, st),
                          'tgmx_pool_rows')  # fmt: skip
            x, ldx, R = a.pooled, D, 1
        _layers(lib, a, x, ldx, R, st)
    elif a.form == _native.DECODER_FORM['pair']:
        _native.check(lib.tgmx_decoder_pair_gemm(a.a1, a.lda1, a.n1, a.ia, a.a2, a.lda2, a.n2, a.ib, a.wa, a.ldwa, D, a.wb, a.ldwb, D, a.mbias, a.merge_act,
                                                 a.h[1], H, a.R, H, a.bad, st), 'tgmx_decoder_pair_gemm')  # fmt: skip
        _layers(lib, a, a.h[1], H, a.R, st)
    else:
        if a.n1 == 0 or a.B == 0:
            return
        _native.check(lib.tgmx_sgemm_nt(a.a1, a.lda1, a.wa, a.ldwa, a.P, 2 * H, a.n1, 2 * H, D, a.mbias, 0, 1, 0, 0, 0, st), 'tgmx_sgemm_nt')
        ly = a.layers[0]
        fuse = a.num_layers == 1 and ly.out <= _native.DECODER_MAX_TAIL and a.merge_act == ACT_RELU
        common = (a.P, 2 * H, a.n1, H, a.ia, a.ib, a.neg, a.idx64, a.off, a.M, a.max_candidates, a.B, a.merge_act)
        if fuse:
            check_supported(lib.tgmx_decoder_score(*common, ly.w, ly.b, ly.out, a.out, 0, a.bad, st), 'tgmx_decoder_score')
            return
        check_supported(lib.tgmx_decoder_score(*common, None, None, 0, a.h[1], H, a.bad, st), 'tgmx_decoder_score')
        _layers(lib, a, a.h[1], H, a.R, st)


__all__ = ['DecoderHead', 'Unsupported', 'build_mlp', 'forward_per_launch', 'linears']
