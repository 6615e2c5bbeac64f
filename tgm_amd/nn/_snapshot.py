"""What the snapshot models (``ChebConv`` / ``GCLSTM``, ``GCNConv`` / ``TGCN``, ``ROLAND``) share on the host: the edge-list conversions, the
counter of skipped edges, and the wrappers of the sparse operators -- a snapshot's CSR by destination ``(indptr, cols, vals, diag)`` from
``tgmx_cheb_laplacian`` or ``tgmx_gcn_norm_csr`` (one sorted-key builder, ``csrc/edge_csr.h``) and the gather SpMM over it."""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import _native
from . import _ops

Csr = Tuple[Tensor, Tensor, Tensor, Tensor]


def _endpoints(edge_index: Tensor) -> Tuple[Tensor, Tensor]:
    """The two rows as contiguous int32 / int64 vectors (an int32 loader batch is read as it is)."""
    _native.require_device(edge_index, 'edge_index')
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f'expected edge_index [2, E], got {list(edge_index.shape)}')
    ei = edge_index if edge_index.dtype in (torch.int64, torch.int32) else edge_index.to(torch.int64)
    src, dst = ei[0], ei[1]
    return (src if src.is_contiguous() else src.contiguous()), (dst if dst.is_contiguous() else dst.contiguous())


def _edge_weight(edge_weight: Optional[Tensor], E: int) -> Optional[Tensor]:
    if edge_weight is None:
        return None
    w = _ops._f32c(edge_weight.detach(), 'edge_weight').reshape(-1)
    if w.numel() != E:
        raise ValueError(f'expected one edge weight per edge ({E}), got {w.numel()}')
    return w


class _Skipped:
    """The device counter of edges skipped for an endpoint outside [0, N), and the ``check()`` that reports it once."""

    def _skipped(self, device) -> Tensor:
        c = self.__dict__.get('_tgmx_skipped')
        if c is None or c.device != device:
            c = self.__dict__['_tgmx_skipped'] = torch.zeros(1, dtype=torch.int32, device=device)
        return c

    def check(self) -> None:
        """Raise if a forward saw an ``edge_index`` entry outside ``[0, num_nodes)`` (such edges are skipped).  Reads the device."""
        c = self.__dict__.get('_tgmx_skipped')
        if c is not None and int(c.item()):
            c.zero_()
            raise ValueError(f'{type(self).__name__}: edge_index held node ids outside [0, num_nodes); those edges were skipped')


def csr_scratch_sizes(E: int, N: int, workspace_bytes: int, who: str) -> List[int]:
    """The five regions of a snapshot's CSR in 4-byte words: indptr, cols, vals, diag and the builder's workspace;
    ``workspace_bytes``: what the builder's ``*_workspace_bytes(E, N)`` answered, 0 for sizes it does not take."""
    if workspace_bytes == 0:
        raise ValueError(f'{who}: {E} edges over {N} nodes are out of range')
    return [N + 1, E, E, N, (workspace_bytes + 3) // 4]


def scaled_laplacian(edge_index: Tensor, edge_weight: Optional[Tensor], N: int, normalization: Optional[str], lam: float, lam_t: Optional[Tensor],
                     skipped: Optional[Tensor] = None, bufs: Optional[List[Tensor]] = None) -> Csr:  # fmt: skip
    """(indptr, cols, vals, diag) of ``tgmx_cheb_laplacian``; ``bufs``: the caller's five regions (indptr, cols, vals, diag, workspace)."""
    lib = _native.load()
    src, dst = _endpoints(edge_index)
    E, dev = src.numel(), src.device
    w = _edge_weight(edge_weight, E)
    sizes = csr_scratch_sizes(E, N, lib.tgmx_cheb_workspace_bytes(E, N), 'ChebConv')
    if bufs is None:
        bufs = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for n in sizes]
    indptr, cols, vals, diag, ws = bufs
    _native.check(
        lib.tgmx_cheb_laplacian(src.data_ptr(), dst.data_ptr(), 1 if src.dtype == torch.int64 else 0, _native.ptr(w), E, N, _native.CHEB_NORM[normalization],
                                lam, _native.ptr(lam_t), indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), ws.data_ptr(),
                                ws.numel() * 4, _native.ptr(skipped), _native.stream_ptr()),
        'tgmx_cheb_laplacian',
    )  # fmt: skip
    return indptr, cols, vals, diag


def propagate_scratch(lap: Csr, C: int) -> Optional[Tensor]:
    """The scratch ``propagate`` splits very long rows (hubs) with; ``None`` when the graph is too small to hold one."""
    n = _native.load().tgmx_cheb_propagate_scratch_floats(lap[1].numel(), C)
    return torch.empty(n, dtype=torch.float32, device=lap[1].device) if n else None


def propagate(lap: Csr, t: Tensor, out: Tensor, prev: Optional[Tensor] = None, alpha: float = 1.0, beta: float = 0.0,
              scratch: Optional[Tensor] = None) -> Tensor:  # fmt: skip
    """out = alpha (L_hat t) + beta prev over 2-D row-major float32 views (column slices of a wider operand are fine)."""
    indptr, cols, vals, diag = lap
    _native.check(
        _native.load().tgmx_cheb_propagate(indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), t.shape[0], t.shape[1], t.data_ptr(),
                                           t.stride(0), _native.ptr(prev), 0 if prev is None else prev.stride(0), alpha, beta, out.data_ptr(),
                                           out.stride(0), cols.numel(), _native.ptr(scratch), 0 if scratch is None else scratch.numel(),
                                           _native.stream_ptr()),
        'tgmx_cheb_propagate',
    )  # fmt: skip
    return out


def gcn_norm_csr(edge_index: Tensor, edge_weight: Optional[Tensor], N: int, fill: float, add_self_loops: bool, skipped: Optional[Tensor] = None,
                 bufs: Optional[List[Tensor]] = None) -> Csr:  # fmt: skip
    """(indptr, cols, vals, diag) of ``tgmx_gcn_norm_csr``: D^-1/2 (A + I) D^-1/2 as a CSR by destination, any number of nodes;
    ``bufs``: the caller's five regions (indptr, cols, vals, diag, workspace)."""
    lib = _native.load()
    src, dst = _endpoints(edge_index)
    E, dev = src.numel(), src.device
    w = _edge_weight(edge_weight, E)
    sizes = csr_scratch_sizes(E, N, lib.tgmx_gcn_workspace_bytes(E, N), 'GCNConv')
    if bufs is None:
        kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.int32)
        bufs = [torch.empty(max(n, 1), dtype=k, device=dev) for n, k in zip(sizes, kinds)]
    indptr, cols, vals, diag, ws = bufs
    _native.check(
        lib.tgmx_gcn_norm_csr(src.data_ptr(), dst.data_ptr(), 1 if src.dtype == torch.int64 else 0, _native.ptr(w), E, N, float(fill),
                              1 if add_self_loops else 0, indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), ws.data_ptr(),
                              ws.numel() * 4, _native.ptr(skipped), _native.stream_ptr()),
        'tgmx_gcn_norm_csr',
    )  # fmt: skip
    return indptr, cols, vals.view(torch.float32), diag


def gcn_propagate(csr: Csr, t: Tensor, out: Tensor, bias: Optional[Tensor] = None, epilogue: str = 'none', prev: Optional[Tensor] = None,
                  tau: Union[float, Tensor] = 0.0, prev_copy: Optional[Tensor] = None, scratch: Optional[Tensor] = None,
                  E: Optional[int] = None) -> Tensor:  # fmt: skip
    """out = epi(A_hat t + bias) over 2-D row-major float32 views (column slices of a wider operand are fine); ``epilogue``: ``'none'``,
    ``'relu'`` or ``'tau'`` (``tau prev + (1 - tau) relu(.)``, ``tau`` a float or a one-element float32 tensor on the device, which is
    not read back).  ``E``: the edge count the CSR was built from when ``cols`` is longer."""
    indptr, cols, vals, diag = csr
    tau_t = tau if isinstance(tau, Tensor) else None
    _native.check(
        _native.load().tgmx_gcn_propagate(indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), t.shape[0], t.shape[1], t.data_ptr(),
                                          t.stride(0), _native.ptr(bias), _native.GCN_EPI[epilogue], _native.ptr(prev),
                                          0 if prev is None else prev.stride(0), 0.0 if tau_t is not None else float(tau), _native.ptr(tau_t),
                                          _native.ptr(prev_copy), 0 if prev_copy is None else prev_copy.stride(0), out.data_ptr(), out.stride(0),
                                          cols.numel() if E is None else E, _native.ptr(scratch), 0 if scratch is None else scratch.numel(),
                                          _native.stream_ptr()),
        'tgmx_gcn_propagate',
    )  # fmt: skip
    return out
