"""DensityOfStateEstimatorHook on host tensors: the numpy path against a dense float64 restatement, its operator against networkx, the probe
signs, the struct mirror and the hook's surface."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tgm_amd import _native
from tgm_amd.hooks import DensityOfStateEstimatorHook, StatelessHook
from tgm_amd.hooks.analytics import dos as D
from tgm_amd.hooks.negatives import counter_u32
from tgm_amd.hooks.registry import list_hooks

GRAPHS = {
    'triangle_tail': ([0, 1, 2, 2, 1], [1, 2, 0, 5, 0]),
    'self_loop': ([4, 4, 9, 7], [4, 9, 7, 4]),
    'random': (np.random.default_rng(0).integers(0, 60, 200).tolist(), np.random.default_rng(1).integers(0, 60, 200).tolist()),
}


def filtered_density(c, n_pts):
    """steps 4 and 5 of the definition, restated: Jackson factors, the integrated series, diff and clip"""
    N = len(c)
    tau = np.pi / (N + 1)
    c = [((N - m + 1) * np.cos(tau * m) + np.sin(tau * m) / np.tan(tau)) / (N + 1) * c[m] for m in range(N)]
    theta = np.arccos(np.linspace(-1 + 1e-8, 1 - 1e-8, n_pts))
    y = c[0] * (theta - np.pi) / 2.0 + sum(c[m] * np.sin(m * theta) / m for m in range(1, N))
    return np.clip(np.diff(-2.0 * y / np.pi), 0, None)


def dense_operator(src, dst):
    ids, (src, dst) = np.unique(src + dst), (np.asarray(src), np.asarray(dst))
    ls, ld = np.searchsorted(ids, src), np.searchsorted(ids, dst)
    A = np.zeros((ids.size, ids.size))
    A[ls, ld] = A[ld, ls] = 1.0
    d = A.sum(1)
    return ids, -A / np.sqrt(np.outer(d, d))


@pytest.mark.parametrize('moments,probes,n_pts', [(20, 100, 1001), (1, 3, 2)])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_host_path_against_the_dense_restatement(name, moments, probes, n_pts):
    src, dst = GRAPHS[name]
    hook = DensityOfStateEstimatorHook(moments, probes, n_pts, seed=11)
    batch = types.SimpleNamespace(edge_src=torch.tensor(src), edge_dst=torch.tensor(dst))
    for call in (1, 2):
        got = hook(None, batch).dos
        ids, S = dense_operator(src, dst)
        Z = D.probe_signs(11, call, ids, probes)
        T = [Z, S @ Z]
        for _ in range(2, max(moments, 2)):
            T.append(2 * (S @ T[-1]) - T[-2])
        want = filtered_density([(Z * t).sum(0).mean() for t in T], n_pts)
        assert got.dtype == np.float64 and got.shape == (n_pts - 1,) and want.max() > 0
        assert np.abs(got - want).max() <= 1e-12 * want.max()
    hook.check()


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_operator_against_networkx(name):
    nx = pytest.importorskip('networkx')
    src, dst = GRAPHS[name]
    ids, indptr, rows, cols, vals = D._operator(np.asarray(src), np.asarray(dst))
    G = nx.from_edgelist(zip(src, dst))
    want = nx.normalized_laplacian_matrix(G, nodelist=sorted(G)).toarray() - np.eye(len(G))
    got = np.zeros_like(want)
    got[rows, cols] = vals
    assert ids.tolist() == sorted(G) and np.array_equal(indptr, np.searchsorted(rows, np.arange(len(G) + 1)))
    assert np.abs(got - want).max() <= 4e-16 and np.abs(got - dense_operator(src, dst)[1]).max() == 0


def test_probe_signs():
    Z = D.probe_signs(123, 4, [0, 5, (1 << 31) - 1], 7)
    assert Z.dtype == np.float64 and Z.shape == (3, 7)
    for r, node in enumerate([0, 5, (1 << 31) - 1]):
        assert Z[r].tolist() == [-1.0 if counter_u32(123, 4, node * 7 + j) >> 31 else 1.0 for j in range(7)]
    big = D.probe_signs(1, 1, np.arange(400), 100)
    assert set(np.unique(big)) == {-1.0, 1.0} and abs(big.mean()) < 4 / np.sqrt(big.size)  # balanced: four sigma of a fair coin
    assert np.array_equal(big, D.probe_signs(1, 1, np.arange(400), 100)) and not np.array_equal(big, D.probe_signs(1, 2, np.arange(400), 100))
    # keyed on the global id: a row does not depend on its neighbours
    assert np.array_equal(D.probe_signs(1, 1, [77], 100)[0], big[77])


def test_struct_mirror_and_envelope():
    lib = _native.load()
    assert lib.tgmx_abi_sizeof(44) == ctypes.sizeof(_native.Dos) > 0
    # the library's envelope also asks for a probe width; the mirror does not: equal at every corner and for every E
    assert all(lib.tgmx_dos_probe_width(E) > 0 for E in range(1, D.MAX_EVENTS + 1))
    for args in [(1, 1, 2, 2), (4096, 1024, 64, 65536), (0, 1, 2, 2), (4097, 1, 2, 2), (1, 1025, 2, 2), (1, 1, 1, 2), (1, 1, 65, 2), (1, 1, 2, 1), (1, 1, 2, 65537)]:
        assert bool(lib.tgmx_dos_supported(*args)) == D.supported(*args) == (lib.tgmx_dos_workspace_bytes(*args) > 0), args
    assert [lib.tgmx_dos_probe_width(E) for E in (0, 1, 200, 4096, 4097)] == [0, 8, 8, 1, 0]


def test_surface():
    import tgm_amd.hooks.analytics as analytics

    assert analytics.DensityOfStateEstimatorHook is D.DensityOfStateEstimatorHook is DensityOfStateEstimatorHook in list_hooks()
    h = DensityOfStateEstimatorHook()
    assert isinstance(h, StatelessHook) and not h.has_state and h.requires == {'edge_src', 'edge_dst'} and h.produces == {'dos'}
    assert (h._moments, h._probing_vectors, h._n_pts, h.sync) == (20, 100, 50, True)
    empty = h(None, types.SimpleNamespace(edge_src=torch.empty(0, dtype=torch.int64), edge_dst=torch.empty(0, dtype=torch.int64))).dos
    assert empty.shape == (49,) and not empty.any()
    for bad in (-2, 1 << 31):  # the device path's predicate: an endpoint outside [0, 2^31) is skipped and flagged
        h = DensityOfStateEstimatorHook(seed=3)
        got = h(None, types.SimpleNamespace(edge_src=torch.tensor([1, bad]), edge_dst=torch.tensor([2, 3]))).dos
        assert np.array_equal(got, DensityOfStateEstimatorHook(seed=3)(None, types.SimpleNamespace(edge_src=torch.tensor([1]), edge_dst=torch.tensor([2]))).dos)
        with pytest.raises(ValueError, match='outside'):
            h.check()
