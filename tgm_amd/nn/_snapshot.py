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


def csr_transpose(csr: Csr, N: int) -> Csr:
    """``tgmx_csr_transpose``: the same matrix as rows by column index; values are copied (bit for bit), ``diag`` is the same tensor."""
    lib = _native.load()
    indptr, cols, vals, diag = csr
    E, dev = cols.numel(), indptr.device
    nbytes = lib.tgmx_csr_transpose_workspace_bytes(E, N)
    if nbytes == 0:
        raise ValueError(f'csr_transpose: {E} entries over {N} nodes are out of range')
    indptr_t = torch.empty(N + 1, dtype=torch.int32, device=dev)
    cols_t = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
    vals_t = torch.empty(max(E, 1), dtype=torch.float32, device=dev)[:E]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _native.check(
        lib.tgmx_csr_transpose(indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), N, E, indptr_t.data_ptr(), cols_t.data_ptr(),
                               vals_t.data_ptr(), None, ws.data_ptr(), nbytes, _native.stream_ptr()),
        'tgmx_csr_transpose',
    )  # fmt: skip
    return indptr_t, cols_t, vals_t, diag


class GCNGraph(_Skipped):
    """One snapshot's normalised adjacency D^-1/2 (A + I) D^-1/2 for ``GCNConv`` / ``TGCN`` on the sparse route: the CSR by destination,
    its transpose (built lazily, once, on the first backward that needs it, then kept), the scratch the propagate splits hub rows with, and
    the counter of skipped edges (``check()``).  Pass it in place of ``edge_index`` (``edge_weight`` then ``None``) to every layer of a
    stack: the snapshot is then sorted once for all layers, and once more for all their backward passes.  Build it with :func:`gcn_graph`.
    The adjacency carries no gradient: edge weights are data."""

    def __init__(self, csr: Optional[Csr], num_nodes: int, E: int, improved: bool, add_self_loops: bool, device, skipped: Optional[Tensor] = None,
                 shared: bool = True) -> None:  # fmt: skip
        self.csr, self.num_nodes, self.E, self.improved, self.add_self_loops, self.device = csr, num_nodes, E, improved, add_self_loops, device
        self.shared = shared  # False: a module built it for one call; the backward then transposes into its own workspace and keeps nothing
        self._t: Optional[Csr] = None
        self._scratch: dict = {}
        if skipped is not None:
            self.__dict__['_tgmx_skipped'] = skipped

    @property
    def skipped(self) -> Tensor:
        return self._skipped(self.device)

    def transposed(self) -> Csr:
        if self._t is None:
            self._t = csr_transpose(self.csr, self.num_nodes)
        return self._t

    def scratch(self, C: int) -> Optional[Tensor]:
        """The hub scratch for a propagate over ``C`` channels (``None``: no row of this graph can be a hub)."""
        if C not in self._scratch:
            n = _native.load().tgmx_cheb_propagate_scratch_floats(self.E, C)
            self._scratch[C] = torch.empty(n, dtype=torch.float32, device=self.device) if n else None
        return self._scratch[C]

    def matches(self, module) -> None:
        if bool(module.improved) != self.improved or bool(module.add_self_loops) != self.add_self_loops:
            raise ValueError(f'{type(module).__name__}(improved={module.improved}, add_self_loops={module.add_self_loops}) was handed a GCNGraph built '
                             f'with improved={self.improved}, add_self_loops={self.add_self_loops}')  # fmt: skip


def gcn_csr_buffers(E: int, N: int, device) -> List[Tensor]:
    """indptr, cols, vals, diag of one snapshot as tensors of their own (a call that saves its CSR for the backward owns them)."""
    flat = torch.empty(2 * N + 1 + 2 * max(E, 1), dtype=torch.int32, device=device)
    indptr, cols, vals, diag = flat.split([N + 1, max(E, 1), max(E, 1), N])
    return [indptr, cols[:E], vals[:E].view(torch.float32), diag.view(torch.float32)]


def gcn_graph(edge_index: Tensor, edge_weight: Optional[Tensor] = None, num_nodes: Optional[int] = None, improved: bool = False,
              add_self_loops: bool = True) -> GCNGraph:  # fmt: skip
    """The :class:`GCNGraph` of a snapshot (``tgmx_gcn_norm_csr``: one sort).  ``num_nodes`` is required: the rows of ``x``."""
    if num_nodes is None or isinstance(num_nodes, bool) or not isinstance(num_nodes, int) or num_nodes <= 0:
        raise ValueError(f'gcn_graph: num_nodes must be a positive int, got {num_nodes!r}')
    src, _ = _endpoints(edge_index)
    E, dev = src.numel(), src.device
    g = GCNGraph(None, num_nodes, E, bool(improved), bool(add_self_loops), dev)
    nbytes = _native.load().tgmx_gcn_workspace_bytes(E, num_nodes)
    sizes = csr_scratch_sizes(E, num_nodes, nbytes, 'gcn_graph')
    ws = torch.empty(sizes[4], dtype=torch.int32, device=dev)
    g.csr = gcn_norm_csr(edge_index, edge_weight, num_nodes, 2.0 if improved else 1.0, add_self_loops, g.skipped, gcn_csr_buffers(E, num_nodes, dev) + [ws])
    return g


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
