"""``LinkPredictor`` (tgm/nn/decoder/linkproppred.py) on HIP kernels: same constructor, ``self.merge`` / ``self.model`` and ``state_dict`` keys.

``forward(z_src, z_dst)`` is the reference's.  Without gradients on the device it is one native call (``tgmx_decoder_forward``, pair
form): the first layer reads the two operands where they are -- no ``[R, 2D]`` concatenation -- and a last layer of at most 16 outputs is
a row dot.  With gradients to track it is the same head as a ``torch.autograd.Function`` (``_decoder_train.py``): one native call that
keeps its activations per call, one native call backward; ``score_pairs`` in the table form likewise, with the gradient of the table.
On the host, or outside the native envelope (parameters that are not contiguous float32, a model that is not the Linear / ReLU chain
the constructor builds, autocast) the same arithmetic runs as torch ops; a merge other than ``ConcatMerge`` / ``LearnableSumMerge`` runs in
torch and the MLP after it natively (with gradients: all of it in torch).

New here, for the evaluation loop of the examples (for every positive edge: index ``z`` twice, concatenate, run the MLP on ``1 + M`` rows):

* :meth:`LinkPredictor.score_pairs` -- ``self(z[src_idx], z[dst_idx])`` without the two gathers;
* :meth:`LinkPredictor.query_one_vs_many` -- every positive against its candidates in one call, the convention of
  ``EdgeBankPredictor.query_one_vs_many``.

Both pick between two forms.  TABLE: ``P = z [W0a ; W0b]^T + [b0 | 0]`` is one GEMM over the ``N'`` rows of the table and a pair costs
``relu(P[a, :H] + P[b, H:])`` dotted with the last layer; PAIR: the gathered GEMM over the ``R`` pairs.  The table form does no more
arithmetic when ``N' <= R``; measured, it stays ahead up to ``N' = 2 R`` (its GEMM runs nearer the MFMA rate than the gathered one):
``N' <= 2 R`` is the default rule; ``TGMX_DECODER_FORM=table|pair`` pins one.  ``TGMX_DECODER_PY=1`` issues the same
launches one ctypes call each.  An index outside ``[0, N')`` is never dereferenced: its score is NaN and :meth:`check` raises once.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from ..core.neg_batch_list import uniform_matrix
from ._decoder_head import DecoderHead, build_mlp, linears
from ._fwd_plumbing import i32, needs_torch
from .aggregation import Aggregator, ConcatMerge, require_aggregator

_INT = (torch.int32, torch.int64)


def _ids(*ts: Tensor) -> List[Tensor]:
    """Contiguous 1-D (or the [B, M] block: row-major) index tensors of ONE dtype: int32 if all are, else int64."""
    dt = torch.int32 if all(t.dtype == torch.int32 for t in ts) else torch.int64
    return [(t if t.dtype == dt else t.to(dt)).contiguous() for t in ts]


class LinkPredictor(DecoderHead, nn.Module):
    """An MLP over merged pairs of node embeddings: ``model(merge(z_src, z_dst)).view(-1)``.

    ``node_dim``: width of the embeddings; ``out_dim``, ``nlayers``, ``hidden_dim``: the MLP (``nlayers = 1`` builds the two Linears of
    ``nlayers = 2``); ``merge_op``: an :class:`Aggregator`, ``ConcatMerge(node_dim)`` by default.
    """

    def __init__(self, node_dim: int, out_dim: int = 1, nlayers: int = 2, hidden_dim: int = 64, merge_op: Optional[Aggregator] = None) -> None:
        super().__init__()
        self.merge = ConcatMerge(dim=node_dim) if merge_op is None else merge_op
        require_aggregator(self.merge)
        self.model = build_mlp(self.merge.out_channels, hidden_dim, out_dim, nlayers)

    # ---- the reference's call ---------------------------------------------------------------------------------------------------------------
    def forward(self, z_src: Tensor, z_dst: Tensor) -> Tensor:
        shaped = z_src.dim() == 2 and z_dst.dim() == 2 and z_src.shape == z_dst.shape
        if shaped and self._train_ready(z_src, z_dst):  # gradients to track: the saving forward, one native call back
            return self._train('pair', None, (-1,), z_src.contiguous(), z_dst.contiguous())
        if not (shaped and self._ready(z_src, z_dst)):
            return self.model(self.merge(z_src, z_dst)).view(-1)
        if self._merge_kind() is None:
            return self._mlp_rows(self.merge(z_src, z_dst).contiguous()).view(-1)
        a1, a2 = z_src.contiguous(), z_dst.contiguous()
        R = a1.shape[0]

        def fill(a, w):
            a.a1, a.lda1, a.n1, a.a2, a.lda2, a.n2 = a1.data_ptr(), a1.stride(0), R, a2.data_ptr(), a2.stride(0), R
            return a1, a2

        return self._run('pair', R, fill, a1.device).view(-1)

    def _ready(self, *zs: Tensor) -> bool:
        """The native head applies: on the device, nothing for autograd to track, float32 everywhere, the constructor's layer chain."""
        if not self._native_ok(*zs):
            return False
        kind = self._merge_kind()
        if kind is None:
            return len(linears(self.model)) <= _native.DECODER_MAX_LAYERS
        return zs[0].shape[1] == self.merge.dim

    def _train_ready(self, *zs: Tensor) -> bool:
        """The native training path applies: :meth:`_ready`'s envelope with something for autograd to track, one of the two shipped merges."""
        return self._trainable(*zs) and self._merge_kind() is not None and zs[0].shape[1] == self.merge.dim

    def _form(self, n_table: int, R: int) -> str:
        H = self.merge.dim if self._merge_kind() == 'sum' else self.model[0].out_features
        if H > _native.DECODER_MAX_H:  # the score kernel keeps a half row in LDS
            return 'pair'
        pinned = os.environ.get('TGMX_DECODER_FORM')
        if pinned in ('table', 'pair'):
            return pinned
        return 'table' if n_table <= 2 * R else 'pair'  # measured: the forms cross between N' = 2 R and 4 R

    # ---- pairs of rows of one table -------------------------------------------------------------------------------------------------------------
    def score_pairs(self, z: Tensor, src_idx: Tensor, dst_idx: Tensor) -> Tensor:
        """What ``self(z[src_idx], z[dst_idx])`` returns, without the two gathers: ``z [N', D]`` holds the batch's unique nodes, the
        indices (int32 or int64, one per pair) point into it."""
        if src_idx.numel() != dst_idx.numel():
            raise ValueError(f'mismatch shape: src_idx: {src_idx.numel()}, dst_idx: {dst_idx.numel()}')
        if (z.dim() == 2 and src_idx.dtype in _INT and dst_idx.dtype in _INT and src_idx.device == z.device and dst_idx.device == z.device
                and src_idx.numel() > 0 and self._train_ready(z) and self._form(z.shape[0], src_idx.numel()) == 'table'):  # fmt: skip
            # gradients to track and the table form: one GEMM over the table forward, its gradient gathered per table row backward
            return self._train('table', tuple(_ids(src_idx.reshape(-1), dst_idx.reshape(-1))), (-1,), z.contiguous())
        if not (z.dim() == 2 and src_idx.dtype in _INT and dst_idx.dtype in _INT and self._ready(z) and self._merge_kind() is not None
                and src_idx.device == z.device and dst_idx.device == z.device):  # fmt: skip
            return self(z[src_idx.reshape(-1).long()], z[dst_idx.reshape(-1).long()])
        R = src_idx.numel()
        return self._pairs(z.contiguous(), R, src_idx.reshape(-1), dst_idx.reshape(-1), None, None, -1, 0, R).view(-1)

    def query_one_vs_many(self, z: Tensor, src_idx: Tensor, dst_idx: Tensor,
                          negatives: Union[Tensor, Sequence[Tensor]]) -> Union[Tensor, List[Tensor]]:  # fmt: skip
        """The evaluation loop's ``B`` decoder calls as one: row ``b`` scores ``(src_idx[b], dst_idx[b])`` in column 0 and
        ``(src_idx[b], negatives[b][m])`` after it -- what ``self(z[src_idx[b].repeat(1 + M)], z[cat([dst_idx[b:b+1], negatives[b]])])`` gives.
        ``negatives`` is ``[B, M]`` (the result is ``[B, 1 + M]``) or a list of ``B`` 1-D index tensors of any lengths, empty ones included
        (the result is a list of ``B`` tensors, views of one buffer).  All indices point into the rows of ``z``.  Nothing is read back."""
        src_idx, dst_idx = src_idx.reshape(-1), dst_idx.reshape(-1)
        B = src_idx.numel()
        if dst_idx.numel() != B:
            raise ValueError(f'mismatch shape: src_idx: {B}, dst_idx: {dst_idx.numel()}')
        as_rows = uniform_matrix(negatives)  # a NegBatchList of equal rows: its matrix, no B-way cat
        if as_rows is not None:
            negatives = as_rows
        ragged = not isinstance(negatives, Tensor)
        if ragged:
            negatives = [t.reshape(-1) for t in negatives]
            if len(negatives) != B:
                raise ValueError(f'negatives holds {len(negatives)} rows for {B} positive edges')
            sizes = [int(t.numel()) for t in negatives]
            if B == 0:
                return []
            neg = torch.cat(negatives) if sum(sizes) else dst_idx[:0]
            R, M, most = B + sum(sizes), 0, max(sizes)
        else:
            if negatives.dim() != 2 or negatives.shape[0] != B:
                raise ValueError(f'negatives must be [B, M] with B = {B}, got {tuple(negatives.shape)}')
            M = int(negatives.shape[1])
            neg, sizes, R, most = negatives.reshape(-1), None, B * (M + 1), M
        out_dim = self.model[-1].out_features
        native = (z.dim() == 2 and all(t.dtype in _INT and t.device == z.device for t in (src_idx, dst_idx, neg)) and self._ready(z)
                  and self._merge_kind() is not None)  # fmt: skip
        if not native:
            # the per-positive loop's pairs, flattened: one call of the torch path
            if ragged:
                reps = torch.tensor([m + 1 for m in sizes], device=src_idx.device)
                ia = torch.repeat_interleave(src_idx.long(), reps)
                ib = torch.cat([torch.cat((dst_idx[b : b + 1].long(), negatives[b].long())) for b in range(B)])
            else:
                ia = src_idx.long().repeat_interleave(M + 1)
                ib = torch.cat((dst_idx.long().unsqueeze(1), negatives.long()), dim=1).reshape(-1)
            # (with gradients to track this method stays on the composed path: only forward / score_pairs have a native backward)
            flat = self.model(self.merge(z[ia], z[ib])).view(-1) if needs_torch(self, 0.0, z) else self(z[ia], z[ib])
        else:
            off = None
            if ragged:
                off_host = np.zeros(B + 1, dtype=np.int64)
                np.cumsum(sizes, out=off_host[1:])
                # host to device, from pinned memory so that the host does not wait: the sizes are shapes, nothing is read back
                off = torch.from_numpy(off_host).pin_memory().to(z.device, non_blocking=True)
            flat = self._pairs(z.contiguous(), R, src_idx, dst_idx, neg, off, M, most, B).view(-1)
        if not ragged:
            return flat.view(B, (M + 1) * out_dim) if as_rows is None else list(flat.view(B, (M + 1) * out_dim).unbind(0))
        return list(torch.split(flat, [(m + 1) * out_dim for m in sizes]))

    def _pairs(self, z: Tensor, R: int, src_idx: Tensor, dst_idx: Tensor, neg: Optional[Tensor], off: Optional[Tensor], M: int, most: int,
               B: int) -> Tensor:  # fmt: skip
        """The native head over pairs of rows of z: flat pairs (M = -1) or B queries with their candidates; returns [R, out_dim]."""
        n_table = z.shape[0]
        form = self._form(n_table, R)
        if form == 'table':
            ids = _ids(src_idx, dst_idx, *(() if neg is None else (neg,)))
            H2 = 2 * (self.merge.dim if self._merge_kind() == 'sum' else self.model[0].out_features)

            def fill(a, w):
                a.a1, a.lda1, a.n1 = z.data_ptr(), z.stride(0), n_table
                a.ia, a.ib, a.neg, a.off = ids[0].data_ptr(), ids[1].data_ptr(), (ids[2].data_ptr() if neg is not None else None), _native.ptr(off)
                a.idx64, a.M, a.max_candidates, a.B = int(ids[0].dtype == torch.int64), M, most, B
                return ids, off

            return self._run('table', R, fill, z.device, scratch=(n_table * H2, 0, 0))
        if M < 0:
            ia, ib = i32(src_idx), i32(dst_idx)
        elif off is None:
            ia = i32(src_idx).repeat_interleave(M + 1)
            ib = torch.cat((i32(dst_idx).unsqueeze(1), i32(neg).view(B, M)), dim=1).reshape(-1)
        else:  # ragged: query b owns rows off[b] + b .. off[b + 1] + b; candidate k of the concatenation sits at k + (its query) + 1
            counts = off[1:] - off[:-1]
            ia = torch.repeat_interleave(i32(src_idx), counts + 1, output_size=R)
            ib = torch.empty(R, dtype=torch.int32, device=z.device)
            ib[off[:-1] + torch.arange(B, device=z.device)] = i32(dst_idx)
            if R > B:
                owner = torch.repeat_interleave(torch.arange(1, B + 1, device=z.device), counts, output_size=R - B)
                ib[torch.arange(R - B, device=z.device) + owner] = i32(neg)

        def fill(a, w):
            a.a1, a.lda1, a.n1, a.a2, a.lda2, a.n2 = z.data_ptr(), z.stride(0), n_table, z.data_ptr(), z.stride(0), n_table
            a.ia, a.ib = ia.data_ptr(), ib.data_ptr()
            return ia, ib

        return self._run('pair', R, fill, z.device)
