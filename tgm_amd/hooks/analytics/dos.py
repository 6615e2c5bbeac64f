"""DensityOfStateEstimatorHook (the hook of the reference's examples/analytics/dos.py): a spectral density-of-states estimate of every
batch's graph by stochastic Chebyshev moments (https://arxiv.org/abs/2305.08750).

The definition, for one batch with endpoints ``edge_src`` / ``edge_dst``:

    graph      G = the simple undirected graph of the endpoint pairs (duplicates and reversed duplicates are one edge), its nodes the ids
               that occur, sorted; A its 0/1 adjacency, a self-loop one 1 on the diagonal; d = A.sum(1)
    operator   S = L_norm - I (the example's ``rescale_matrix(L, lo=0, hi=2)``): every stored entry, the diagonal included, is
               S_ij = -A_ij / sqrt(d_i d_j)
    moments    nM = max(moments, 2); Z [n, nZ] of +-1; T_0 = Z, T_1 = S Z, T_m = 2 S T_{m-1} - T_{m-2}; c_m = mean_j sum_i Z_ij (T_m)_ij
               (c_0 = n: the estimate is not normalised by n, as the reference's is not)
    filter     c_m <- g_m c_m, g_m = ((N - m + 1) cos(tau m) + sin(tau m) / tan(tau)) / (N + 1), N = nM, tau = pi / (N + 1)
    density    x = linspace(-1 + 1e-8, 1 - 1e-8, n_pts), theta = arccos x, y = c_0 (theta - pi) / 2 + sum_{m >= 1} c_m sin(m theta) / m,
               cdf = -2 y / pi, dos = clip(diff(cdf), min=0), of length n_pts - 1

The reference draws Z from numpy's global stream, which no device can reproduce.  Here Z is defined over the counter-based generator of
csrc/common.h, as the negative samplers and dropout are: ``Z[node, j] = +1`` if bit 31 of ``counter_u32(seed, call, node_id * nZ + j)`` is
clear, else ``-1`` (``probe_signs``), with ``seed`` the hook's ``seed=`` or ``torch.initial_seed()`` and ``call`` the hook's call counter
(1 for the first batch).  Keyed on the global node id, the estimate does not depend on how nodes are numbered locally.  Parity with the
reference is therefore parity of the definition given Z, not of its random stream.

On a ROCm device a batch of up to 4096 events is one ``tgmx_dos_estimate`` call (csrc/dos.hip: the batch's graph sorted, deduplicated and
kept in LDS, the recurrence in float32 with float64 sums, three launches).  A snapshot of 4097 to 2^22 events -- a day or a week of a stream
-- is one ``tgmx_dos_large_estimate`` call (csrc/dos_large.hip: the graph as a CSR in HBM, the same recurrence and sums, a workgroup per slab
of probe columns); ``TGMX_DOS_LARGE=torch`` sends that range to the composed path instead (``native`` is the default).  With ``sync=True``
``batch.dos`` is a float64 numpy array as the reference's, the call's one read; with ``sync=False`` (extension, BatchAnalyticsHook's
convention) a float64 device tensor, nothing read back.  Outside both envelopes (more than 2^22 events, more than 1024 probes, more than 64
moments, more than 65536 points) the device path is ``_estimate_composed``: the same definition from stock torch ops in float32 over a dense
[n, n] operator.  Host tensors run it over numpy in float64.  An empty batch gives zeros of length ``n_pts - 1`` (our choice: the reference
raises on networkx's null graph).  An event with an endpoint outside [0, 2^31) is skipped, on every path; ``check()`` raises if a batch
carried one.  ``last_path`` names the route of the last call: 'lds', 'csr', 'composed', 'host' or 'empty'.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from ... import _native
from ...core import DGBatch, DGraph
from ..base import StatelessHook
from ..negatives import _M64, counter_u32
from ..registry import hook
from .batch_analytics import _native_vector, require_on

MAX_EVENTS, MAX_PROBES, MAX_MOMENTS, MAX_POINTS = 4096, 1024, 64, 65536  # tgmx_dos_supported
MAX_EVENTS_LARGE = 1 << 22  # tgmx_dos_large_supported


def supported(E: int, nZ: int, nM: int, n_pts: int) -> bool:
    """The kernel's envelope (``tgmx_dos_supported``, mirrored: the choice of path needs no library).  The library also asks that a probe
    width fits LDS (``tgmx_dos_probe_width(E) > 0``), true for every E up to ``MAX_EVENTS`` as the kernel is built; tests/test_dos_cpu.py
    holds the two together."""
    return 1 <= E <= MAX_EVENTS and 1 <= nZ <= MAX_PROBES and 2 <= nM <= MAX_MOMENTS and 2 <= n_pts <= MAX_POINTS


def large_supported(E: int, nZ: int, nM: int, n_pts: int) -> bool:
    """The CSR route's envelope (``tgmx_dos_large_supported``, mirrored; tests/test_dos_large_cpu.py holds the two together)."""
    return MAX_EVENTS < E <= MAX_EVENTS_LARGE and 1 <= nZ <= MAX_PROBES and 2 <= nM <= MAX_MOMENTS and 2 <= n_pts <= MAX_POINTS


def _large_route() -> str:
    route = os.environ.get('TGMX_DOS_LARGE', 'native')
    if route not in ('native', 'torch'):
        raise ValueError(f"TGMX_DOS_LARGE must be 'native' or 'torch' (got {route!r})")
    return route


def probe_signs(seed: int, call: int, node_ids, nZ: int) -> np.ndarray:
    """Z [n, nZ] float64 of +-1: +1 where bit 31 of ``counter_u32(seed, call, node_id * nZ + j)`` is clear."""
    ids = np.asarray(node_ids).astype(np.uint64).reshape(-1, 1)
    index = ids * np.uint64(nZ) + np.arange(nZ, dtype=np.uint64)
    # the generator xors its three inputs before it mixes: seed and call folded here, in Python integers, leave an array-only call
    folded = counter_u32(((seed & _M64) ^ ((call & _M64) * 0x9E3779B97F4A7C15)) & _M64, 0, index)
    return np.where((folded >> np.uint64(31)) & np.uint64(1), -1.0, 1.0)


def _operator(src: np.ndarray, dst: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(node_ids [n], indptr [n + 1], rows [nnz], cols [nnz], vals [nnz]) of S = L_norm - I in CSR order, float64."""
    s, d = src.astype(np.int64), dst.astype(np.int64)
    keys = np.unique(np.concatenate([(s << 32) | d, (d << 32) | s]))
    node_ids, rows = np.unique(keys >> 32, return_inverse=True)
    cols = np.searchsorted(node_ids, keys & 0xFFFFFFFF)
    deg = np.bincount(rows, minlength=node_ids.size).astype(np.float64)
    indptr = np.concatenate([[0], np.cumsum(deg.astype(np.int64))])
    return node_ids, indptr, rows, cols, -1.0 / np.sqrt(deg[rows] * deg[cols])


def jackson(c: np.ndarray) -> np.ndarray:
    N = c.shape[0]
    m = np.arange(N)
    tau = np.pi / (N + 1)
    return ((N - m + 1) * np.cos(tau * m) + np.sin(tau * m) / np.tan(tau)) / (N + 1) * c


def density(c: np.ndarray, n_pts: int) -> np.ndarray:
    """dos [n_pts - 1] from the filtered moments: the Chebyshev series integrated to a cdf, differenced and clipped."""
    theta = np.arccos(np.linspace(-1 + 1e-8, 1 - 1e-8, n_pts))
    m = np.arange(1, len(c))
    y = c[0] * (theta - np.pi) / 2.0 + np.sum(c[m, None] * np.sin(m[:, None] * theta) / m[:, None], 0)
    return np.diff(y * (-2.0 / np.pi)).clip(min=0)


def _counter_u32_torch(folded_seed: int, index: torch.Tensor) -> torch.Tensor:
    """counter_u32(folded_seed, 0, index) over an int64 tensor: int64 products wrap like uint64 ones, a logical shift is an arithmetic one
    masked."""
    signed = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    lsr = lambda x, k: (x >> k) & ((1 << (64 - k)) - 1)
    x = (index * signed(0xD1B54A32D192ED03)) ^ signed(folded_seed)
    x = x + signed(0x9E3779B97F4A7C15)
    x = (x ^ lsr(x, 30)) * signed(0xBF58476D1CE4E5B9)
    x = (x ^ lsr(x, 27)) * signed(0x94D049BB133111EB)
    x = x ^ lsr(x, 31)
    return lsr(x, 32)


@hook
class DensityOfStateEstimatorHook(StatelessHook):
    """Computes Density of States (DOS): https://arxiv.org/abs/2305.08750.  ``seed`` (extension): the probes' seed, default
    ``torch.initial_seed()`` read at the first batch.  ``sync=False`` (extension): ``batch.dos`` stays a float64 tensor on the batch's device.
    """

    _cls_requires = {'edge_src', 'edge_dst'}
    _cls_produces = {'dos'}

    def __init__(self, moments: int = 20, probing_vectors: int = 100, n_pts: int = 50, seed: Optional[int] = None, sync: bool = True) -> None:
        super().__init__()
        if moments < 1 or probing_vectors < 1 or n_pts < 2:
            raise ValueError(f'DensityOfStateEstimatorHook: moments >= 1, probing_vectors >= 1 and n_pts >= 2 (got {moments}, {probing_vectors}, {n_pts})')
        self._moments, self._probing_vectors, self._n_pts = int(moments), int(probing_vectors), int(n_pts)
        self._seed = seed
        self._rng_seed: Optional[int] = None
        self.sync = bool(sync)
        self.calls = 0  # never reset: a second epoch probes differently
        self._ws: Optional[torch.Tensor] = None
        self._status: Optional[torch.Tensor] = None
        self._bad_host = False
        self.last_path: Optional[str] = None  # 'lds' | 'csr' | 'composed' | 'host' | 'empty'
        self.__post_init__()

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        src, dst = batch.edge_src, batch.edge_dst
        if (src is None) != (dst is None) or (src is not None and src.numel() != dst.numel()):
            raise ValueError('DensityOfStateEstimatorHook needs edge_src and edge_dst of one length')
        if self._rng_seed is None:
            self._rng_seed = (self._seed if self._seed is not None else torch.initial_seed()) & _M64
        self.calls += 1
        E = 0 if src is None else int(src.numel())
        device = src.device if src is not None else torch.device('cpu')
        shape = (E, self._probing_vectors, max(self._moments, 2), self._n_pts)
        if E == 0:
            self.last_path, out = 'empty', torch.zeros(self._n_pts - 1, dtype=torch.float64, device=device)
        elif device.type != 'cuda':
            self.last_path, out = 'host', torch.from_numpy(self._estimate_host(src, dst))
        elif supported(*shape):
            self.last_path, out = 'lds', self._estimate_device(src, dst, large=False)
        elif large_supported(*shape) and _large_route() == 'native':
            self.last_path, out = 'csr', self._estimate_device(src, dst, large=True)
        else:
            self.last_path, out = 'composed', self._estimate_composed(src, dst)
        self.add_batch_attribute(batch, 'dos', out.cpu().numpy() if self.sync else out)  # sync: the one read of the batch
        return batch

    def _estimate_device(self, src: torch.Tensor, dst: torch.Tensor, large: bool) -> torch.Tensor:
        """One C call, nothing read back: ``tgmx_dos_estimate`` (the graph in LDS) or ``tgmx_dos_large_estimate`` (the graph as a CSR)."""
        device = src.device
        require_on(device, 'DensityOfStateEstimatorHook', edge_src=src, edge_dst=dst)
        src, dst = _native_vector(src, 'edge_src'), _native_vector(dst, 'edge_dst')
        lib = _native.load()
        a = _native.DosLarge() if large else _native.Dos()
        workspace_bytes, estimate = (lib.tgmx_dos_large_workspace_bytes, lib.tgmx_dos_large_estimate) if large else (lib.tgmx_dos_workspace_bytes, lib.tgmx_dos_estimate)
        a.src, a.dst, a.E = src.data_ptr(), dst.data_ptr(), src.numel()
        a.src_is64, a.dst_is64 = int(src.dtype == torch.int64), int(dst.dtype == torch.int64)
        a.nZ, a.nM, a.n_pts = self._probing_vectors, max(self._moments, 2), self._n_pts
        a.seed, a.call = self._rng_seed, self.calls
        nbytes = int(workspace_bytes(a.E, a.nZ, a.nM, a.n_pts))
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if self._status is None or self._status.device != device:
            self._status = torch.zeros(1, dtype=torch.int64, device=device)
        out = torch.empty(self._n_pts - 1, dtype=torch.float64, device=device)
        a.dos, a.status, a.workspace, a.workspace_bytes = out.data_ptr(), self._status.data_ptr(), self._ws.data_ptr(), self._ws.numel()
        rc = estimate(ctypes.byref(a), _native.stream_ptr(device.index))
        if rc:
            _native.check(rc, 'tgmx_dos_large_estimate' if large else 'tgmx_dos_estimate')
        return out

    def _valid(self, s, d):
        """Host and composed paths: which events take part (both endpoints in [0, 2^31), the kernel's predicate); a batch that carried
        another is noted (the device path's status word)."""
        keep = (s >= 0) & (d >= 0) & (s < (1 << 31)) & (d < (1 << 31))
        if not bool(keep.all()):
            self._bad_host = True
        return keep

    def _estimate_host(self, src: torch.Tensor, dst: torch.Tensor) -> np.ndarray:
        """The definition over numpy, float64 throughout."""
        s, d = src.detach().numpy().reshape(-1), dst.detach().numpy().reshape(-1)
        keep = self._valid(s, d)
        nM = max(self._moments, 2)
        if not keep.any():
            return np.zeros(self._n_pts - 1)
        node_ids, indptr, _, cols, vals = _operator(s[keep], d[keep])
        Z = probe_signs(self._rng_seed, self.calls, node_ids, self._probing_vectors)
        apply = lambda T: np.add.reduceat(vals[:, None] * T[cols], indptr[:-1], axis=0)  # every row holds an entry
        c = np.empty((nM, Z.shape[1]))
        prev, cur = Z, apply(Z)
        c[0], c[1] = (Z * prev).sum(0), (Z * cur).sum(0)
        for m in range(2, nM):
            prev, cur = cur, 2 * apply(cur) - prev
            c[m] = (Z * cur).sum(0)
        return density(jackson(c.mean(1)), self._n_pts)

    def _estimate_composed(self, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """The definition from stock torch ops on the batch's device: a dense [n, n] float32 operator, float32 recurrence, the column sums
        and what follows in float64.  The fallback outside the kernel's envelope, and the baseline tools/bench_dos.py times."""
        dev, nZ, nM = src.device, self._probing_vectors, max(self._moments, 2)
        s, d = src.reshape(-1).long(), dst.reshape(-1).long()
        keep = self._valid(s, d)
        s, d = s[keep], d[keep]
        ids = torch.unique(torch.cat([s, d]))
        n = ids.numel()
        if n == 0:
            return torch.zeros(self._n_pts - 1, dtype=torch.float64, device=dev)
        ls, ld = torch.searchsorted(ids, s), torch.searchsorted(ids, d)
        A = torch.zeros(n, n, dtype=torch.float32, device=dev)
        one = torch.ones((), dtype=torch.float32, device=dev)
        A.index_put_((ls, ld), one)
        A.index_put_((ld, ls), one)
        deg = A.sum(1)
        S = -A / torch.sqrt(deg[:, None] * deg[None, :])
        folded = ((self._rng_seed & _M64) ^ ((self.calls & _M64) * 0x9E3779B97F4A7C15)) & _M64
        bits = _counter_u32_torch(folded, ids[:, None] * nZ + torch.arange(nZ, device=dev))
        Z = 1.0 - 2.0 * ((bits >> 31) & 1).to(torch.float32)
        prev, cur = Z, S @ Z
        c = [(Z * prev).sum(0, dtype=torch.float64), (Z * cur).sum(0, dtype=torch.float64)]
        for _ in range(2, nM):
            prev, cur = cur, 2 * (S @ cur) - prev
            c.append((Z * cur).sum(0, dtype=torch.float64))
        c = torch.stack(c).mean(1)
        m = torch.arange(nM, dtype=torch.float64, device=dev)
        tau = math.pi / (nM + 1)
        c = ((nM - m + 1) * torch.cos(tau * m) + torch.sin(tau * m) / math.tan(tau)) / (nM + 1) * c
        theta = torch.arccos(torch.linspace(-1 + 1e-8, 1 - 1e-8, self._n_pts, dtype=torch.float64, device=dev))
        y = c[0] * (theta - math.pi) / 2.0 + (c[1:, None] * torch.sin(m[1:, None] * theta) / m[1:, None]).sum(0)
        return torch.diff(y * (-2.0 / math.pi)).clamp(min=0)

    def check(self) -> None:
        """Raise if a batch carried an id outside [0, 2^31) (its event took no part).  One read of the device's status word."""
        bad = self._bad_host or (self._status is not None and int(self._status.item()) & _native.AN_BAD_ID)
        if bad:
            raise ValueError('DensityOfStateEstimatorHook: a batch carried an id outside [0, 2^31); its event was skipped')
