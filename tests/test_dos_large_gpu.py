"""DensityOfStateEstimatorHook past 4096 events (csrc/dos_large.hip: the graph as a CSR in HBM) against a plain float64 sparse restatement of
its definition, at the project's forward bar: max |dos - dos_f64| <= 1e-5 max(dos_f64).

Measured on one MI355X, as a fraction of max(dos_f64), the worse of the two id dtypes (equal bits, in fact): see DESIGN.md, "Snapshots".
"""
import functools
import types

import numpy as np
import pytest
import torch

from tgm_amd import _native
from tgm_amd.hooks import DensityOfStateEstimatorHook
from tgm_amd.hooks.analytics.dos import probe_signs

pytestmark = pytest.mark.gpu
SEED = 5


def dos_f64(src, dst, moments, probes, n_pts):
    keys = np.unique(np.concatenate([(src << 32) | dst, (dst << 32) | src]))
    ids, rows = np.unique(keys >> 32, return_inverse=True)
    cols = np.searchsorted(ids, keys & 0xFFFFFFFF)
    deg = np.bincount(rows).astype(np.float64)
    vals, starts = -1.0 / np.sqrt(deg[rows] * deg[cols]), np.searchsorted(rows, np.arange(ids.size))
    S = lambda T: np.add.reduceat(vals[:, None] * T[cols], starts, axis=0)
    Z = probe_signs(SEED, 1, ids, probes)
    T, c = [Z, S(Z)], np.zeros(max(moments, 2))
    for m in range(c.size):
        if m >= 2:
            T = [T[1], 2 * S(T[1]) - T[0]]
        c[m] = (Z * T[min(m, 1)]).sum(0).mean()
    k, tau = np.arange(c.size), np.pi / (c.size + 1)
    c = ((c.size - k + 1) * np.cos(tau * k) + np.sin(tau * k) / np.tan(tau)) / (c.size + 1) * c
    theta = np.arccos(np.linspace(-1 + 1e-8, 1 - 1e-8, n_pts))
    y = c[0] * (theta - np.pi) / 2.0 + sum(c[m] * np.sin(m * theta) / m for m in range(1, c.size))
    return np.diff(y * (-2.0 / np.pi)).clip(min=0)


def random_batch(E, ids, seed=2):  # tests/test_dos_gpu.py's: self-loops and reversed repeats among uniform pairs
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, ids, E), rng.integers(0, ids, E)
    dst[: E // 20] = src[: E // 20]
    src[E // 2 : E // 2 + E // 10], dst[E // 2 : E // 2 + E // 10] = dst[: E // 10].copy(), src[: E // 10].copy()
    return src, dst


def star(leaves, hub=1 << 20):
    return np.full(leaves, hub), hub + 1 + 3 * np.arange(leaves)


def heavy_tail():
    u = np.random.default_rng(3).random((2, 30000))
    return (9000 * u[0] ** 3).astype(np.int64), 9000 + (9000 * u[1] ** 2).astype(np.int64)


def both(*graphs):
    return tuple(np.concatenate(v) for v in zip(*graphs))


def path(delta):  # around the switch between T in LDS and T in the workspace, for the 8 probes the case runs with
    lds_rows = _native.load().tgmx_dos_large_lds_rows
    n = lds_rows(1 << 20, 8) + delta
    assert n - 1 > 4096 and lds_rows(n - 1, 8) == n - delta  # of that call's E
    return 7 + np.arange(n - 1), 8 + np.arange(n - 1)


GRAPHS = {  # name: (graph, probes)
    'first_past_lds': (lambda: random_batch(4097, 8000), 100),
    'tiny_n': (lambda: random_batch(20000, 300), 100),
    'heavy_tail': (heavy_tail, 16),
    'hub_beside_random': (lambda: both(star(5000), random_batch(4000, 3000)), 16),
    'star70000': (lambda: both(star(70000), random_batch(100, 3000)), 8),
    'path_lds_rows-1': (lambda: path(-1), 8), 'path_lds_rows': (lambda: path(0), 8), 'path_lds_rows+1': (lambda: path(1), 8),
    'largest_id_self_loop': (lambda: both(random_batch(4097, 8000), (np.array([(1 << 31) - 1]),) * 2), 100),
}  # fmt: skip


@functools.lru_cache(maxsize=None)
def case(name, moments=20, probes=None, n_pts=1001):
    make, default_probes = GRAPHS[name]
    src, dst = make()
    return src, dst, dos_f64(src, dst, moments, probes or default_probes, n_pts)


def run(src, dst, dtype=torch.int64, moments=20, probes=100, n_pts=1001, sync=True, path='csr'):
    hook = DensityOfStateEstimatorHook(moments, probes, n_pts, seed=SEED, sync=sync)
    out = hook(None, types.SimpleNamespace(edge_src=torch.from_numpy(src).to('cuda', dtype), edge_dst=torch.from_numpy(dst).to('cuda', dtype))).dos
    assert hook.last_path == path
    hook.check()
    return out


def assert_close(got, want):
    assert got.dtype == np.float64 and got.shape == want.shape
    err = np.abs(got - want).max()
    print(f'max error {err:.3e}, {err / want.max():.3e} of the maximum {want.max():.4f}')
    assert err <= 1e-5 * want.max()


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_graph_shapes(name, dtype):
    src, dst, want = case(name)
    assert_close(run(src, dst, dtype, probes=GRAPHS[name][1]), want)


EDGES = {  # PV: the slab width of the default call; 101, 130 and 257 probes end in a partial slab at the rule's widths 2, 4 and 8
    'probes1': lambda pv: dict(probes=1), 'probesPV-1': lambda pv: dict(probes=max(pv - 1, 1)), 'probesPV': lambda pv: dict(probes=pv),
    'probesPV+1': lambda pv: dict(probes=pv + 1), 'probes101': lambda pv: dict(probes=101), 'probes130': lambda pv: dict(probes=130),
    'probes257': lambda pv: dict(probes=257), 'moments2': lambda pv: dict(moments=2), 'moments64': lambda pv: dict(moments=64),
    'n_pts2': lambda pv: dict(n_pts=2), 'n_pts50': lambda pv: dict(n_pts=50),
}  # fmt: skip


@pytest.mark.parametrize('edge', sorted(EDGES))
def test_parameter_edges(edge):
    width = _native.load().tgmx_dos_large_probe_width
    assert [width(4097, p) for p in (101, 130, 257)] == [2, 4, 8]
    kw = EDGES[edge](width(4097, 100))
    src, dst, want = case('first_past_lds', **kw)
    assert_close(run(src, dst, **kw), want)


def test_interface(monkeypatch):
    src, dst, want = case('first_past_lds')
    a, b = run(src, dst), run(src, dst, torch.int32)
    assert np.array_equal(a, b)  # equal (seed, call): equal bits, whatever the id dtype
    t = run(src, dst, sync=False)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), a)
    hook = DensityOfStateEstimatorHook(20, 100, 1001, seed=SEED)
    bad = types.SimpleNamespace(edge_src=torch.from_numpy(np.append(src, -1)).cuda(), edge_dst=torch.from_numpy(np.append(dst, 6)).cuda())
    assert np.array_equal(hook(None, bad).dos, a) and hook.last_path == 'csr'  # the event with the negative id took no part
    with pytest.raises(ValueError, match='outside'):
        hook.check()
    monkeypatch.setenv('TGMX_DOS_LARGE', 'torch')
    assert_close(run(src, dst, path='composed'), want)
