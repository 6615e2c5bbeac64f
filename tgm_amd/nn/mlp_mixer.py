"""``FeedForwardNet`` / ``MLPMixer`` (tgm/nn/modules/mlp_mixer.py; same constructors and parameter names: ``token_norm``,
``token_feedforward.ffn.{0,3}``, ``channel_norm``, ``channel_feedforward.ffn.{0,3}``) on HIP kernels.

Inference (no gradient needed, and no active dropout) runs natively inside the token kernel's envelope: ``tgmx_mixer_token`` does the
whole token-mixing block of a seed -- LayerNorm over the K tokens, Linear K -> Ht = int(f_t K), exact-erf GELU, Linear -> K, residual -- and
also writes the channel LayerNorm of its result; the channel FFN is two exact-fp32 MFMA GEMMs with a GELU and a residual epilogue
(``tgmx_sgemm_nt_ep``, ``csrc/dense.hip``).  The envelope: a seed's tile, ``4 * (K C + (K + Ht) * 128)`` bytes, fits 64 KiB of LDS (K = 20,
Ht = 10: C <= 627).  Outside it the kernel answers ``TGMX_E_UNSUPPORTED`` and inference is the composed torch arithmetic below, under
``torch.no_grad()`` (a ``RuntimeWarning`` says so, once per module).

Training: ``MLPMixer.forward`` under gradients is native inside the training envelope (``_graphmixer_train.py``: float32 input on the
parameters' device, no autocast, contiguous float32 parameters, the tile inside both token kernels' LDS -- the forward's bound and
``4 * (4 K + 2 Ht) * 33`` bytes for the backward's narrowest pass): the forward's launches with the token block's dropout sites in the kernel, and a backward of
``tgmx_mixer_token_backward`` plus dense GEMMs and reductions, with ``dx`` for an input that asks for it.  Train mode with dropout > 0 draws
counter-based masks (``tgmx_dropout_t``).  Outside the envelope, with ``TGMX_GRAPHMIXER_BWD=torch``, and for ``FeedForwardNet`` on its own, the
reference arithmetic is composed from torch ops on the device under autograd, with the same parameters.  CPU tensors raise
``NativeLibraryError``.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .. import _native
from . import _ops
from ._fwd_plumbing import Unsupported, check_supported, needs_torch


class FeedForwardNet(nn.Module):
    r"""Two-layered MLP with GELU activation (Linear -> GELU -> Dropout -> Linear -> Dropout)."""

    def __init__(self, input_dim: int, dim_expansion_factor: float, dropout: float = 0.0) -> None:
        super().__init__()
        self.input_dim, self.dim_expansion_factor, self.dropout = input_dim, dim_expansion_factor, dropout
        hidden = int(dim_expansion_factor * input_dim)
        self.ffn = nn.Sequential(nn.Linear(input_dim, hidden), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden, input_dim), nn.Dropout(dropout))

    def forward(self, X: Tensor) -> Tensor:
        _native.require_device(X, 'FeedForwardNet input')
        if needs_torch(self, self.dropout, X):
            return self.ffn(X)  # training: torch ops under autograd (not native)
        x = _ops._f32c(X, 'FeedForwardNet input')
        lin0, lin1 = self.ffn[0], self.ffn[3]
        M, C, H = x.numel() // self.input_dim, self.input_dim, lin0.out_features
        h = torch.empty((M, H), dtype=torch.float32, device=x.device)
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        sgemm_ep(x.view(M, C), lin0.weight.detach(), h, lin0.bias.detach(), act=2)
        sgemm_ep(h, lin1.weight.detach(), out.view(M, C), lin1.bias.detach())
        return out


def sgemm_ep(A: Tensor, B: Tensor, out: Tensor, bias=None, act: int = 0, res=None) -> Tensor:
    """out[M, N] = act(A[M, K] @ B[N, K].T + bias) + res; act 0 none, 1 ReLU, 2 exact-erf GELU (row-major 2-D views)."""
    lib = _native.load()
    M, K, N = A.shape[0], A.shape[1], B.shape[0]
    _native.check(
        lib.tgmx_sgemm_nt_ep(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), out.stride(0), M, N, K, _native.ptr(bias), act,
                             _native.ptr(res), 0 if res is None else res.stride(0), _native.stream_ptr()),
        'tgmx_sgemm_nt_ep',
    )  # fmt: skip
    return out


def warn_composed(module: nn.Module, who: str, why: str) -> None:
    """Once per module: inference left the native path."""
    if not module.__dict__.get('_tgmx_warned'):
        module.__dict__['_tgmx_warned'] = True
        warnings.warn(f'tgm_amd {who}: inference runs as torch ops on the device, not natively: {why}', RuntimeWarning, stacklevel=3)


def token_block(mixer: 'MLPMixer', x: Tensor, ldx: int, S: int, z1: Tensor, y: Tensor, ldo: int) -> None:
    """``tgmx_mixer_token`` with ``mixer``'s token FFN and channel LayerNorm (x, z1, y: device pointers' owners, rows of ldx / ldo floats).
    Raises ``Unsupported`` (nothing launched, z1 / y untouched) when the seed's tile does not fit the kernel's 64 KiB of LDS."""
    lib = _native.load()
    tn, cn, tf = mixer.token_norm, mixer.channel_norm, mixer.token_feedforward.ffn
    K, C = mixer.num_tokens, mixer.num_channels
    check_supported(
        lib.tgmx_mixer_token(x.data_ptr(), ldx, S, K, C, tn.weight.data_ptr(), tn.bias.data_ptr(), tf[0].weight.data_ptr(), tf[0].bias.data_ptr(),
                             tf[0].out_features, tf[3].weight.data_ptr(), tf[3].bias.data_ptr(), cn.weight.data_ptr(), cn.bias.data_ptr(),
                             float(tn.eps), z1.data_ptr(), y.data_ptr(), ldo, _native.stream_ptr()),
        'tgmx_mixer_token',
    )  # fmt: skip


class MLPMixer(nn.Module):
    r"""MLP-Mixer block (https://openreview.net/forum?id=ayPPc0SyLv1, Eq. 6): token mixing over the K tokens of each channel, then
    channel mixing over the C channels of each token, each as ``x + FFN(LayerNorm(x))``.

    Input / output: [B, K, C] = [batch, num_tokens, num_channels].  Inference is native inside the token kernel's LDS envelope (see the
    module docstring; composed outside it); with gradients enabled the forward and ``backward()`` are native inside the training envelope
    (dropout included) and the reference arithmetic composed from torch ops on the device outside it.
    """

    def __init__(self, num_tokens: int, num_channels: int, token_dim_expansion_factor: float = 0.5, channel_dim_expansion_factor: float = 4.0,
                 dropout: float = 0.0) -> None:  # fmt: skip
        super().__init__()
        self.num_tokens, self.num_channels, self.dropout = num_tokens, num_channels, dropout
        self.token_norm = nn.LayerNorm(num_tokens)
        self.token_feedforward = FeedForwardNet(input_dim=num_tokens, dim_expansion_factor=token_dim_expansion_factor, dropout=dropout)
        self.channel_norm = nn.LayerNorm(num_channels)
        self.channel_feedforward = FeedForwardNet(input_dim=num_channels, dim_expansion_factor=channel_dim_expansion_factor, dropout=dropout)

    def forward(self, node_x: Tensor) -> Tensor:
        _native.require_device(node_x, 'MLPMixer input')
        if node_x.dim() != 3 or node_x.shape[1] != self.num_tokens or node_x.shape[2] != self.num_channels:
            raise ValueError(f'MLPMixer expects [B, {self.num_tokens}, {self.num_channels}], got {list(node_x.shape)}')
        if needs_torch(self, self.dropout, node_x):
            from . import _graphmixer_train  # (imports this module)

            if _graphmixer_train.mixer_in_envelope(self, node_x):
                return _graphmixer_train.apply_mixer(self, node_x)
            return self._torch_forward(node_x)
        return self._native_forward(node_x)

    def _torch_forward(self, x: Tensor) -> Tensor:
        """The reference arithmetic from torch ops (autograd-capable; not native)."""
        h = F.layer_norm(x.permute(0, 2, 1), (self.num_tokens,), self.token_norm.weight, self.token_norm.bias, self.token_norm.eps)
        z = x + self.token_feedforward.ffn(h).permute(0, 2, 1)
        h = F.layer_norm(z, (self.num_channels,), self.channel_norm.weight, self.channel_norm.bias, self.channel_norm.eps)
        return z + self.channel_feedforward.ffn(h)

    def _check_native(self) -> None:
        if self.token_norm.eps != self.channel_norm.eps:
            raise NotImplementedError('tgm_amd MLPMixer: the native token block takes one LayerNorm eps for both norms')
        if not (self.token_norm.elementwise_affine and self.channel_norm.elementwise_affine and self.token_norm.bias is not None
                and self.channel_norm.bias is not None):
            raise NotImplementedError('tgm_amd MLPMixer: the native token block needs affine LayerNorms with bias')  # fmt: skip
        for p in self.parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise NotImplementedError('tgm_amd MLPMixer: parameters must be contiguous float32')

    def _native_forward(self, node_x: Tensor) -> Tensor:
        self._check_native()
        x = _ops._f32c(node_x, 'MLPMixer input')
        B, K, C = x.shape
        R = B * K
        f32 = dict(dtype=torch.float32, device=x.device)
        z1, y = torch.empty((R, C), **f32), torch.empty((R, C), **f32)
        try:
            token_block(self, x, C, B, z1, y, C)
        except Unsupported as e:  # the seed's tile does not fit tgmx_mixer_token's LDS: compose
            warn_composed(self, 'MLPMixer', str(e))
            with torch.no_grad():
                return self._torch_forward(x)
        cf = self.channel_feedforward.ffn
        h = torch.empty((R, cf[0].out_features), **f32)
        sgemm_ep(y, cf[0].weight.detach(), h, cf[0].bias.detach(), act=2)
        out = torch.empty((B, K, C), **f32)
        sgemm_ep(h, cf[3].weight.detach(), out.view(R, C), cf[3].bias.detach(), res=z1)
        return out
