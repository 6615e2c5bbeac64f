"""DensityOfStateEstimatorHook on the device (csrc/dos.hip) against a plain float64 restatement of its definition over a dense operator,
at the project's forward bar: max |dos - dos_f64| <= 1e-5 max(dos_f64)."""
import functools
import types

import numpy as np
import pytest
import torch

from tgm_amd import DGData, DGDataLoader, DGraph, _native
from tgm_amd.hooks import DensityOfStateEstimatorHook, HookManager
from tgm_amd.hooks.analytics.dos import probe_signs

pytestmark = pytest.mark.gpu
SEED = 5


def dos_f64(src, dst, call, moments, probes, n_pts):
    ids = np.unique(np.concatenate([src, dst]))
    ls, ld = np.searchsorted(ids, src), np.searchsorted(ids, dst)
    A = np.zeros((ids.size, ids.size))
    A[ls, ld] = A[ld, ls] = 1.0
    d = A.sum(1)
    S = -A / np.sqrt(np.outer(d, d))
    Z = probe_signs(SEED, call, ids, probes)
    nM = max(moments, 2)
    c = np.zeros((nM, probes))
    prev, cur = Z, S @ Z
    c[0], c[1] = (Z * prev).sum(0), (Z * cur).sum(0)
    for m in range(2, nM):
        prev, cur = cur, 2 * (S @ cur) - prev
        c[m] = (Z * cur).sum(0)
    c = c.mean(1)
    k = np.arange(nM)
    tau = np.pi / (nM + 1)
    c = ((nM - k + 1) * np.cos(tau * k) + np.sin(tau * k) / np.tan(tau)) / (nM + 1) * c
    theta = np.arccos(np.linspace(-1 + 1e-8, 1 - 1e-8, n_pts))
    y = c[0] * (theta - np.pi) / 2.0 + sum(c[m] * np.sin(m * theta) / m for m in range(1, nM))
    return np.diff(y * (-2.0 / np.pi)).clip(min=0)


def star(deg):
    return np.full(deg, 1 << 20), (1 << 20) + 1 + 3 * np.arange(deg)


def path(n):
    return 7 + np.arange(n - 1), 8 + np.arange(n - 1)


def random_batch(E, ids, seed):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, ids, E), rng.integers(0, ids, E)
    dst[: E // 20] = src[: E // 20]  # self-loops
    src[E // 2 : E // 2 + E // 10], dst[E // 2 : E // 2 + E // 10] = dst[: E // 10].copy(), src[: E // 10].copy()  # reversed repeats
    return src, dst


GRAPHS = {
    'one_edge': lambda: (np.array([3]), np.array([9])),
    'self_loop': lambda: (np.array([(1 << 31) - 1]), np.array([(1 << 31) - 1])),
    'path63': lambda: path(63), 'path64': lambda: path(64), 'path65': lambda: path(65),
    'star70': lambda: star(70), 'star300': lambda: star(300),
    'two_stars': lambda: tuple(np.concatenate(v) for v in zip(star(70), (np.full(130, 5), 1000 + np.arange(130)))),  # two chunked rows
    'wiki200': lambda: random_batch(200, 300, 0),
    'comment4096': lambda: random_batch(4096, 8000, 1),
    'beyond4097': lambda: random_batch(4097, 8000, 2),  # outside the envelope: the composed path
}  # fmt: skip


@functools.lru_cache(maxsize=None)
def case(name, moments=20, probes=100, n_pts=1001):
    src, dst = GRAPHS[name]()
    return src, dst, dos_f64(src, dst, 1, moments, probes, n_pts)


def run(src, dst, dtype=torch.int64, moments=20, probes=100, n_pts=1001, sync=True, hook=None):
    hook = hook or DensityOfStateEstimatorHook(moments, probes, n_pts, seed=SEED, sync=sync)
    batch = types.SimpleNamespace(edge_src=torch.from_numpy(src).to('cuda', dtype), edge_dst=torch.from_numpy(dst).to('cuda', dtype))
    out = hook(None, batch).dos
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
    assert_close(run(src, dst, dtype), want)


def test_repeats_and_reversed_repeats_are_one_edge():
    one = run(np.array([3]), np.array([9]))
    assert np.array_equal(run(np.array([3, 9, 3]), np.array([9, 3, 9])), one) and one.max() > 0


def test_parameter_edges():
    pv = _native.load().tgmx_dos_probe_width(200)
    assert pv > 1
    src, dst, _ = case('wiki200')
    for kw in [dict(probes=p) for p in (1, pv - 1, pv, pv + 1)] + [dict(moments=m) for m in (1, 2, 3, 64)] + [dict(n_pts=n) for n in (2, 50)]:
        assert_close(run(src, dst, **kw), case('wiki200', **kw)[2])
    assert np.array_equal(run(src, dst, moments=1), run(src, dst, moments=2))


def test_interface():
    src, dst, _ = case('wiki200')
    a, b = run(src, dst), run(src, dst, torch.int32)
    assert np.array_equal(a, b)  # equal (seed, call): equal bits
    t = run(src, dst, sync=False)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), a)
    empty = run(src[:0], dst[:0], n_pts=50)
    assert empty.shape == (49,) and not empty.any()
    hook = DensityOfStateEstimatorHook(seed=SEED)
    skipped = hook(None, types.SimpleNamespace(edge_src=torch.tensor([4, -1], device='cuda'), edge_dst=torch.tensor([5, 6], device='cuda'))).dos
    assert np.array_equal(skipped, run(np.array([4]), np.array([5]), n_pts=50))  # the event with the negative id took no part
    with pytest.raises(ValueError, match='outside'):
        hook.check()


def test_through_the_loader():
    src, dst = random_batch(120, 40, 3)
    edges = torch.from_numpy(np.stack([src, dst], 1)).int()
    dg = DGraph(DGData.from_raw(torch.arange(120), edges), device='cuda:0')
    hook = DensityOfStateEstimatorHook(moments=8, probing_vectors=16, n_pts=33, seed=SEED)
    hm = HookManager(keys=['dos'])
    hm.register('dos', hook)
    hm.set_active_hooks('dos')
    seen = [(b.edge_src.cpu().numpy(), b.edge_dst.cpu().numpy(), b.dos) for b in DGDataLoader(dg, batch_size=40, hook_manager=hm)]
    assert len(seen) == 3 and hook.calls == 3
    for call, (s, d, dos) in enumerate(seen, 1):  # batch k probes with call k
        assert_close(dos, dos_f64(s, d, call, 8, 16, 33))
    again = DensityOfStateEstimatorHook(moments=8, probing_vectors=16, n_pts=33, seed=SEED)
    again.calls = 1
    assert not np.array_equal(run(seen[0][0], seen[0][1], hook=again), seen[0][2])  # the same batch as call 2: other probes
