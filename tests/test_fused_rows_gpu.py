"""Row runs of the fused hop-0 + hop-1 launch (G > 0 hop-1 rows of one hop-0 seed per wave: TGMX_FUSED_ROWS / tgmx_set_fused_rows)
against the default schedule (0: one wave per hop-1 row).  Two identical pipelines run in lockstep over the same stream, the
schedule switched around each one's calls; every output tensor must be bit-identical.  Every case runs an explicit G > 0."""

import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _stream(seed, N, E, D, tmax, hubs=0):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    if hubs:  # half the edges end at one of `hubs` nodes
        pick = torch.rand((E,), generator=g) < 0.5
        dst = torch.where(pick, torch.randint(0, hubs, (E,), generator=g, dtype=torch.int32), dst)
    ts = torch.sort(torch.randint(1, tmax, (E,), generator=g, dtype=torch.int64)).values
    x = torch.rand((E, D), generator=g) if D else None
    return src, dst, ts, x


def _graph(src, dst, ts, x):
    from tgm_amd import DGData, DGraph

    return DGraph(DGData.from_raw(ts, torch.stack([src, dst], 1), x), device=DEV)


def _loader(dg, N, ks, bs, pool=1, mode='ring', **kw):
    from tgm_amd import DGDataLoader
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook

    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(0, N, seed=5))
    hook = RecencyNeighborHook(N, ks, ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time'], mode=mode, validate='deferred',
                               batch_size=bs if mode == 'csr' else None, **kw)
    hm.register('k', hook)
    if pool is None:
        return hm, hook, DGDataLoader(dg, batch_size=bs, hook_manager=hm)
    return hm, hook, DGDataLoader(dg, batch_size=bs, hook_manager=hm, output_pool=pool)


def _tensors(batch):
    """Every tensor the batch carries, by name (hop lists flattened; by-id features as their edge ids)."""
    out = {}
    for name in dir(batch):
        if name.startswith('_'):
            continue
        try:
            v = getattr(batch, name)
        except Exception:
            continue
        if isinstance(v, torch.Tensor):
            out[name] = v
        elif isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                if isinstance(t, torch.Tensor):
                    out[f'{name}[{i}]'] = t
                elif hasattr(t, 'eids'):
                    for j, e in enumerate(t.eids):
                        out[f'{name}[{i}].eids[{j}]'] = e
    return out


def _same(a, b, tag):
    ta, tb = _tensors(a), _tensors(b)
    assert ta.keys() == tb.keys(), tag
    assert any(k.startswith('nbr_nids') for k in ta), f'{tag}: no neighbour outputs'
    for k in ta:
        assert ta[k].shape == tb[k].shape and ta[k].dtype == tb[k].dtype, f'{tag} {k}'
        assert torch.equal(ta[k], tb[k]), f'{tag} {k}'


@contextlib.contextmanager
def _rows(value):
    from tgm_amd import _native

    lib = _native.load()
    lib.tgmx_set_fused_rows(value)
    try:
        yield
    finally:
        lib.tgmx_set_fused_rows(-1)  # back to TGMX_FUSED_ROWS / the library's default


def _lockstep(dg, N, ks, bs, rows, pool=1, n_batches=None, check=None, reset_at=None, epochs=1, **kw):
    """Pipeline A on one wave per hop-1 row, B on `rows` > 0 hop-1 rows per wave, batch by batch."""
    assert rows > 0
    (hma, ha, la), (hmb, hb, lb) = _loader(dg, N, ks, bs, pool, **kw), _loader(dg, N, ks, bs, pool, **kw)
    seen = 0
    with hma.activate('k'), hmb.activate('k'):
        for ep in range(epochs):
            ia, ib = iter(la), iter(lb)
            b = 0
            while n_batches is None or b < n_batches:
                if reset_at is not None and b == reset_at:
                    ha.reset_state()
                    hb.reset_state()
                with _rows(0):
                    xa = next(ia, None)
                with _rows(rows):
                    xb = next(ib, None)
                if xa is None:
                    assert xb is None
                    break
                if check is None or check(b):
                    _same(xa, xb, f'G={rows} epoch {ep} batch {b}')
                    seen += 1
                del xa, xb
                b += 1
    ha.check()
    hb.check()
    if kw.get('mode', 'ring') == 'ring':
        assert torch.equal(ha._ring, hb._ring), 'rings'
        assert torch.equal(ha._write_pos, hb._write_pos), 'write_pos'
    assert seen > 0
    return seen


@pytest.mark.parametrize('delta', ['1', '0'])
def test_cfg2_full_size_benched_window(delta, monkeypatch):
    """The headline shape (bench.py's stream, bs 200, k = [20, 20], D = 172, pool of one, 'deferred') up to the end of the timed
    window of `bench.py --steps 20 --warmup 5` (batches 394 - 413), with delta feature writes on and off."""
    from tgm_amd.synth import make_stream

    monkeypatch.setenv('TGMX_DELTA_WRITES', delta)
    torch.manual_seed(1337)
    st = make_stream('wiki', seed=1337)
    dg = _graph(st.src.cpu(), st.dst.cpu(), st.ts.cpu(), st.edge_x.cpu())
    _lockstep(dg, st.num_nodes, [20, 20], 200, 4, n_batches=414, check=lambda b: b >= 394 or b % 64 == 0)


def test_cfg2_default_loader_arguments():
    from tgm_amd.synth import make_stream

    torch.manual_seed(1337)
    st = make_stream('wiki', seed=1337)
    dg = _graph(st.src.cpu(), st.dst.cpu(), st.ts.cpu(), st.edge_x.cpu())
    _lockstep(dg, st.num_nodes, [20, 20], 200, 3, pool=None, n_batches=40)


@pytest.mark.parametrize('rows', [1, 2, 3, 4, 5, 20])
def test_rows_per_wave(rows):
    dg = _graph(*_stream(3, 500, 6000, 64, 40_000))
    _lockstep(dg, 500, [20, 20], 100, rows)


@pytest.mark.parametrize('ks,rows', [([15, 20], 4), ([15, 20], 2), ([20, 10], 3), ([20, 10], 4), ([7, 7], 5), ([7, 7], 4), ([8, 20], 3)])
def test_k0_not_divisible_and_b_above_k(ks, rows):
    # B = max(ks): [20, 10], [8, 20] and the k0 = 15 rows look up windows wider than their k
    dg = _graph(*_stream(5, 700, 7000, 72, 50_000))
    _lockstep(dg, 700, ks, 120, rows)


@pytest.mark.parametrize('rows', [4, 3])
def test_edge_features_by_id(rows):
    dg = _graph(*_stream(13, 600, 5000, 8, 4000))
    _lockstep(dg, 600, [10, 10], 100, rows, edge_features='by_id')


@pytest.mark.parametrize('rows', [4, 3])
def test_static_index_wide_rows(rows):
    dg = _graph(*_stream(17, 600, 6000, 64, 30_000))
    _lockstep(dg, 600, [20, 20], 100, rows, mode='csr')
    _lockstep(dg, 600, [15, 10], 100, rows, mode='csr')


@pytest.mark.parametrize('rows', [4, 3])
def test_directed_and_hubs(rows):
    dg = _graph(*_stream(19, 400, 6000, 72, 2000, hubs=3))
    _lockstep(dg, 400, [20, 20], 150, rows, directed=True)
    _lockstep(dg, 400, [20, 20], 150, rows)


@pytest.mark.parametrize('rows', [4, 3])
def test_reset_with_deferral_pending_and_epoch_restart(rows):
    dg = _graph(*_stream(11, 800, 6000, 64, 5000))
    _lockstep(dg, 800, [10, 10], 100, rows, reset_at=17, epochs=2)
