"""Host plumbing the native inference forwards share (GraphMixer, DyGFormer, TPNet, TGCN, the MLPMixer modules): index conversions,
the "take the composed path" decisions, the scratch buffer kept between batches, the argument block cached against the parameters'
versions, and the input checks of the pair encoders.  Nothing here launches a kernel."""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native
from . import _ops
from ._paramver import TransientCaches, param_key, param_list


def up4(n: int) -> int:
    """n rounded up to a multiple of 4 floats: a 16-byte aligned leading dimension for the GEMM operands."""
    return (n + 3) // 4 * 4


def i32(t: Tensor) -> Tensor:
    return t if (t.dtype == torch.int32 and t.is_contiguous()) else t.to(torch.int32).contiguous()


def i64(t: Tensor) -> Tensor:
    return t if (t.dtype == torch.int64 and t.is_contiguous()) else t.to(torch.int64).contiguous()


def ids(t: Tensor) -> Tensor:
    """int32 / int64 are read in place; anything else (floating tensors of integral values, narrow integers) goes through .long()"""
    if t.dtype not in (torch.int32, torch.int64):
        t = t.long()
    return t.contiguous()


def pow2ceil(n: int) -> int:
    return 1 << max(1, (int(n) - 1).bit_length())


class Unsupported(RuntimeError):
    """A native entry point answered TGMX_E_UNSUPPORTED: the caller takes the composed path."""


def check_supported(rc: int, what: str) -> None:
    if rc == _native.E_UNSUPPORTED:
        msg = _native.load().tgmx_last_error()
        raise Unsupported(f'{what}: {msg.decode() if msg else "unsupported"}')
    _native.check(rc, what)


def needs_torch(module: nn.Module, dropout: float, *inputs: Tensor) -> bool:
    """The composed torch path: autograd has something to track, or dropout is active."""
    if module.training and dropout > 0:
        return True
    if not torch.is_grad_enabled():
        return False
    # param_list caches in the module's __dict__, and only TransientCaches modules leave that cache behind on pickle / deepcopy
    params = param_list(module) if isinstance(module, TransientCaches) else module.parameters()
    return any(t.requires_grad for t in inputs) or any(p.requires_grad for p in params)


_GRANULE = 64  # floats (256 bytes): every region starts as aligned as the buffer itself, a 16-byte aligned GEMM operand at the least


def carve_scratch(owner: nn.Module, sizes: Sequence[int], device) -> List[Tensor]:
    """One float32 view per entry of ``sizes`` (in floats, each rounded up to the granule) into ONE buffer that ``owner`` keeps between
    calls; the buffer is regrown when it is too small or lives on another device, and is never empty."""
    sizes = [(n + _GRANULE - 1) // _GRANULE * _GRANULE for n in sizes]
    total = sum(sizes)
    ws = owner.__dict__.get('_tgmx_ws')
    if ws is None or ws.numel() < max(1, total) or ws.device != device:
        ws = owner.__dict__['_tgmx_ws'] = torch.empty(max(1, total), dtype=torch.float32, device=device)
    return list(ws[:total].split(sizes))


def weight_keeper() -> Tuple[list, Callable[..., int]]:
    """(keep, f32): ``f32(t, what)`` is the device pointer of ``t`` as contiguous float32; ``keep`` holds the tensors behind the pointers."""
    keep: list = []

    def f32(t: Tensor, what: str = 'weight') -> int:
        keep.append(_ops._f32c(t.detach(), what))
        return keep[-1].data_ptr()

    return keep, f32


def cached_weights(owner: nn.Module, build: Callable[[], object]):
    """What ``build()`` makes of ``owner``'s parameters (stacked weights, an argument block), cached on ``owner`` against their versions."""
    d = owner.__dict__
    key = param_key(owner)
    if d.get('_tgmx_wkey') != key:
        d['_tgmx_w'] = build()
        d['_tgmx_wkey'] = key
    return d['_tgmx_w']


def cached_block(owner: nn.Module, build: Callable[[Callable[..., int]], object]) -> tuple:
    """(argument block with the weights filled in, the tensors it points at), cached on ``owner`` against its parameters' versions;
    ``build(f32)`` makes the block, taking every weight pointer from ``f32``."""

    def block():
        keep, f32 = weight_keeper()
        return build(f32), keep

    return cached_weights(owner, block)


def fill_mixer_layers(blk, mixers: Iterable[nn.Module], f32: Callable[..., int], who: str) -> float:
    """Fill ``blk.layers[i]`` (``tgmx_mixer_layer_t``) from the i-th ``MLPMixer``; returns the LayerNorm eps all of them share."""
    mixers = list(mixers)
    eps = float(mixers[0].token_norm.eps) if mixers else 1e-5
    for ly, m in zip(blk.layers, mixers):
        tf, cf = m.token_feedforward.ffn, m.channel_feedforward.ffn
        if float(m.token_norm.eps) != eps:
            raise NotImplementedError(f'tgm_amd {who}: the native forward takes one LayerNorm eps for every layer')
        ly.tok_g, ly.tok_b, ly.ch_g, ly.ch_b = f32(m.token_norm.weight), f32(m.token_norm.bias), f32(m.channel_norm.weight), f32(m.channel_norm.bias)
        ly.tok_w1, ly.tok_b1, ly.tok_w2, ly.tok_b2 = f32(tf[0].weight), f32(tf[0].bias), f32(tf[3].weight), f32(tf[3].bias)
        ly.ch_w1, ly.ch_b1, ly.ch_w2, ly.ch_b2 = f32(cf[0].weight), f32(cf[0].bias), f32(cf[3].weight), f32(cf[3].bias)
        ly.tok_hidden, ly.ch_hidden = tf[0].out_features, cf[0].out_features
    return eps


def pair_inputs(node_x: Tensor, src: Tensor, dst: Tensor, edge_time: Tensor, nids: Tensor, nbr_t: Tensor, nbr_x: Tensor, src_rows: Optional[Tensor],
                dst_rows: Optional[Tensor], node_dim: int, edge_dim: int, check_slots: Callable[[int], None], n: str) -> dict:  # fmt: skip
    """The checked, converted inputs of a pair encoder (``forward`` with identity rows, or ``encode_pairs`` with row indices into hop 0 of
    the sampler's batch).  ``check_slots(k)`` is the encoder's own rule on the k neighbour slots per row; ``n`` names the pair count in
    the messages."""
    if nids.dim() != 2 or nbr_x.dim() != 3 or tuple(nbr_t.shape) != tuple(nids.shape) or tuple(nbr_x.shape[:2]) != tuple(nids.shape):
        raise ValueError(f'expected neighbour ids / times [S, k] and edge features [S, k, d], got {list(nids.shape)}, {list(nbr_t.shape)}, {list(nbr_x.shape)}')
    check_slots(nids.shape[1])
    if nbr_x.shape[2] != edge_dim or node_x.dim() != 2 or node_x.shape[1] != node_dim:
        raise ValueError(f'expected node_x [N, {node_dim}] and edge features of width {edge_dim}, got {list(node_x.shape)} and '
                         f'{list(nbr_x.shape)}')
    for name, t in (('node_x', node_x), ('src', src), ('dst', dst), ('edge_time', edge_time), ('neighbours', nids), ('neighbours_time', nbr_t),
                    ('neighbours_edge_feat', nbr_x)):  # fmt: skip
        _native.require_device(t, name)
    count = src.numel()
    if dst.numel() != count or edge_time.numel() != count:
        raise ValueError('src, dst and edge_time must have one entry per pair')
    if src_rows is None:
        if nids.shape[0] < 2 * count:
            raise ValueError(f'{count} pairs need neighbour rows [:{n}] for the sources and [{n}:2{n}] for the destinations, got {nids.shape[0]} rows')
    else:
        _native.require_device(src_rows, 'src_rows')
        _native.require_device(dst_rows, 'dst_rows')
        if src_rows.numel() != count or dst_rows.numel() != count:
            raise ValueError('src_rows and dst_rows must have one entry per pair')
        src_rows, dst_rows = i32(src_rows.reshape(-1)), i32(dst_rows.reshape(-1))
    return dict(node_x=_ops._f32c(node_x, 'node_x'), src=i32(src.reshape(-1)), dst=i32(dst.reshape(-1)), t=i64(edge_time.reshape(-1)),
                nids=i32(nids), nbr_t=i64(nbr_t), nbr_x=_ops._f32c(nbr_x, 'neighbours_edge_feat'), src_rows=src_rows, dst_rows=dst_rows)  # fmt: skip
