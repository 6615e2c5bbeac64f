"""Deferred ring commit (tgmx_recency_step_t.defer): a deferring hook and its non-deferring twin (defer_commit = False) over the same
stream must give bit-identical outputs for every batch, and the same ring state once the pending commit is flushed."""

import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _stream(seed, N, E, D, tmax):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    ts = torch.sort(torch.randint(1, tmax, (E,), generator=g, dtype=torch.int64)).values
    x = torch.rand((E, D), generator=g) if D else None
    return src, dst, ts, x


def _graph(src, dst, ts, x):
    from tgm_amd import DGData, DGraph

    return DGraph(DGData.from_raw(ts, torch.stack([src, dst], 1), x), device=DEV)


def _hook(N, ks, defer, directed=False, key_arith='int32', edge_features='dense', neg=True):
    from tgm_amd.hooks import RecencyNeighborHook

    keys, tkeys = (['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']) if neg else (['edge_src', 'edge_dst'], ['edge_time', 'edge_time'])
    h = RecencyNeighborHook(N, ks, keys, tkeys, mode='ring', key_arith=key_arith, validate='deferred', directed=directed, edge_features=edge_features)
    h.defer_commit = defer
    return h


def _loader(dg, N, ks, bs, defer, pool, world=1, rank=0, **kw):
    from tgm_amd import DGDataLoader
    from tgm_amd.dist import EdgeShardHook
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook

    hm = HookManager(keys=['k'])
    if world > 1:  # a rank's share of every batch (the rings replay the whole batch: m = 2 bs)
        hm.register('k', EdgeShardHook(rank, world))
        hm.register('k', RandomNegativeEdgeSamplerHook(0, N, seed=5, like='shard_dst', time_key='shard_time'))
        hook = RecencyNeighborHook(N, ks, ['shard_src', 'shard_dst', 'neg'], ['shard_time', 'shard_time', 'neg_time'], mode='ring', validate='deferred', **kw)
        hook.defer_commit = defer
    else:
        hm.register('k', RandomNegativeEdgeSamplerHook(0, N, seed=5))
        hook = _hook(N, ks, defer, **kw)
    hm.register('k', hook)
    return hm, hook, DGDataLoader(dg, batch_size=bs, hook_manager=hm, output_pool=pool)


def _deferred(h) -> int:
    """Batches whose commit the hook deferred so far (0 without a deferred-commit state)."""
    from tgm_amd import _native

    return int(_native.load().tgmx_defer_count(h._defer)) if h._defer is not None else 0


def _same_batch(a, b, L, tag):
    for h in range(L):
        assert torch.equal(a.nbr_nids[h], b.nbr_nids[h]), f'{tag} hop {h} ids'
        assert torch.equal(a.nbr_edge_time[h], b.nbr_edge_time[h]), f'{tag} hop {h} times'
        xa, xb = a.nbr_edge_x[h], b.nbr_edge_x[h]
        if hasattr(xa, 'eids'):  # edge_features='by_id': the edge ids behind the slots
            xa, xb = xa.eids[h], xb.eids[h]
        if isinstance(xa, torch.Tensor):
            assert torch.equal(xa, xb), f'{tag} hop {h} features'


def _same_state(h1, h2, B):
    r1, r2 = h1._ring, h2._ring  # (the properties flush)
    assert torch.equal(r1, r2), 'rings'
    assert torch.equal(h1._write_pos, h2._write_pos), 'write_pos'
    if h1._ring_x is not None:
        live = r1.view(torch.int32).view(-1, 4)[:, 0] >= 0  # nbr of every slot
        assert torch.equal(h1._ring_x[live], h2._ring_x[live]), 'ring_x of live slots'


def _lockstep(dg, N, ks, bs, pool, n_batches=None, reset_at=None, epochs=1, world=1, **kw):
    """A deferring hook and its twin per rank, all in lockstep; every batch of the deferring hooks must actually defer."""
    pairs = [(_loader(dg, N, ks, bs, True, pool, world, r, **kw), _loader(dg, N, ks, bs, False, pool, world, r, **kw)) for r in range(world)]
    hms = [hm for pr in pairs for (hm, _, _) in pr]
    hooks = [(a[1], b[1]) for a, b in pairs]
    seen = 0
    with contextlib.ExitStack() as stack:
        for hm in hms:
            stack.enter_context(hm.activate('k'))
        for ep in range(epochs):
            for b, xs in enumerate(zip(*[ld for pr in pairs for (_, _, ld) in pr])):
                if n_batches is not None and b == n_batches:
                    break
                if reset_at is not None and b == reset_at:
                    for h1, h2 in hooks:
                        h1.reset_state()
                        h2.reset_state()
                for r in range(world):
                    _same_batch(xs[2 * r], xs[2 * r + 1], len(ks), f'rank {r} epoch {ep} batch {b}')
                seen += 1
                del xs
    for h1, h2 in hooks:
        h1.check()
        h2.check()
        assert _deferred(h1) >= seen, f'only {_deferred(h1)} of {seen} batches deferred their commit'
        assert _deferred(h2) == 0
        _same_state(h1, h2, max(ks))
    return hooks


def test_cfg2_full_size_loader_pool1():
    from tgm_amd.synth import make_stream

    st = make_stream('wiki', seed=1337)
    dg = _graph(st.src.cpu(), st.dst.cpu(), st.ts.cpu(), st.edge_x.cpu())
    _lockstep(dg, st.num_nodes, [20, 20], 200, 1, n_batches=120)


# every shape takes the fused plan (rows too wide for the packed narrow-row kernel: k1 * D / 4 > 8 * lanes per seed), so every
# batch defers; the twin takes the commit launch
@pytest.mark.parametrize(
    'N,E,D,tmax,ks,bs,directed,key_arith',
    [
        (300, 6000, 64, 50_000, [10, 10], 100, False, 'int32'),
        (3000, 8000, 64, 3_000_000, [10, 10], 64, False, 'int32'),  # int32 key wrap: runs of one node split (the header's CAS fold)
        (3000, 8000, 64, 3_000_000, [10, 10], 64, False, 'int64'),
        (40, 6000, 64, 300, [20, 20], 200, False, 'int32'),  # hubs: c = B entries of a node in one batch, heavy time ties
        (400, 6000, 72, 2000, [8, 8], 150, True, 'int32'),  # directed
        (3000, 8000, 64, 2_600_000, [20, 20], 400, False, 'int32'),  # m = 800: a rider per chunk (three-phase placement, coherent copies)
        (2000, 4096, 72, 2_600_000, [8, 8], 512, False, 'int32'),  # m = 1024: the largest batch that defers
    ],
)
def test_twin_random(N, E, D, tmax, ks, bs, directed, key_arith):
    dg = _graph(*_stream(7, N, E, D, tmax))
    _lockstep(dg, N, ks, bs, 1, directed=directed, key_arith=key_arith)


def test_reset_mid_stream_and_epoch_restart():
    dg = _graph(*_stream(11, 800, 6000, 64, 5000))
    _lockstep(dg, 800, [10, 10], 100, 1, reset_at=17, epochs=2)


def test_edge_features_by_id():
    dg = _graph(*_stream(13, 600, 5000, 8, 4000))
    _lockstep(dg, 600, [10, 10], 100, 1, edge_features='by_id')


def test_hook_by_hook_with_non_qualifying_calls():
    """Direct hook calls: store slices defer; a batch that is not a slice of the store (a copy) and a 'sync' call flush first."""
    from tgm_amd import DGDataLoader

    N, ks = 500, [10, 10]
    dg = _graph(*_stream(17, N, 5000, 64, 3000))
    h1, h2 = _hook(N, ks, True, neg=False), _hook(N, ks, False, neg=False)
    for b, batch in enumerate(DGDataLoader(dg, batch_size=100)):
        if b % 7 == 3:  # not a slice of the store: the deferring hook commits what is pending, then runs without deferral
            batch.edge_time = batch.edge_time.clone()
        if b % 11 == 5:
            h1._validate = h2._validate = 'sync'
        x = h1(dg, batch)
        xs = [tuple(t.clone() for t in (x.nbr_nids[h], x.nbr_edge_time[h], x.nbr_edge_x[h])) for h in range(2)]
        y = h2(dg, batch)
        for h in range(2):
            assert torch.equal(xs[h][0], y.nbr_nids[h]) and torch.equal(xs[h][1], y.nbr_edge_time[h]), f'batch {b} hop {h}'
            assert torch.equal(xs[h][2], y.nbr_edge_x[h]), f'batch {b} hop {h} features'
        h1._validate = h2._validate = 'deferred'
        if b % 9 == 4:
            _same_state(h1, h2, 10)
    assert 0 < _deferred(h1) < 50 and _deferred(h2) == 0
    _same_state(h1, h2, 10)


def test_pending_entry_time_equals_next_query_time():
    """Every edge of batch t + 1 carries the last time of batch t: its queries see (ts < q) exactly the entries still pending."""
    N, E, bs = 200, 4000, 100
    src, dst, _, x = _stream(19, N, E, 64, 10)
    ts = torch.repeat_interleave(torch.arange(E // bs, dtype=torch.int64), bs) * 2
    ts[bs - 1::bs] += 2  # the last edge of batch t has the time of batch t + 1
    dg = _graph(src, dst, ts, x)
    _lockstep(dg, N, [10, 10], bs, 1)


def test_two_ranks_on_one_gpu():
    """Two ranks' hooks in one process (a deferred-commit state each), a 400-edge global batch: every ring replays m = 800 entries."""
    dg = _graph(*_stream(23, 3000, 8000, 64, 2_600_000))
    _lockstep(dg, 3000, [20, 20], 400, 1, world=2)


def test_switching_deferral_off_mid_stream():
    dg = _graph(*_stream(29, 600, 5000, 64, 4000))
    hm1, h1, ld1 = _loader(dg, 600, [10, 10], 100, True, 1)
    hm2, h2, ld2 = _loader(dg, 600, [10, 10], 100, False, 1)
    with hm1.activate('k'), hm2.activate('k'):
        for b, (x, y) in enumerate(zip(ld1, ld2)):
            if b == 20:
                n = _deferred(h1)
                h1.defer_commit = False  # commits what is pending; later batches take the commit launch
            _same_batch(x, y, 2, f'batch {b}')
    assert n >= 20 and h1._defer is None
    _same_state(h1, h2, 10)
