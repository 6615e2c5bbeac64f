"""Row order of the fused hop-0 + hop-1 launch (TGMX_FUSED_ORDER / tgmx_set_fused_order: 1 deals the seeds across the seed groups,
2 also runs every seed's newest quad of rows first) against the identity order (0).  Identical pipelines run in lockstep over one
stream, the order switched around each one's calls; every batch tensor must be bit-identical to mode 0's.  Every case runs at
least six consecutive batches on a pool of one, so that the spans carried in out_valid from call to call -- read at the top of the
wave since this order exists -- decide what is written."""

import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SRC_DST_NEG = (['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time'])
SRC_DST = (['edge_src', 'edge_dst'], ['edge_time', 'edge_time'])
SRC = (['edge_src'], ['edge_time'])


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


def _loader(dg, N, ks, bs, keys, mode='ring', defer=True, **kw):
    from tgm_amd import DGDataLoader
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook

    hm = HookManager(keys=['k'])
    if 'neg' in keys[0]:
        hm.register('k', RandomNegativeEdgeSamplerHook(0, N, seed=5))
    hook = RecencyNeighborHook(N, ks, keys[0], keys[1], mode=mode, validate='deferred', batch_size=bs if mode == 'csr' else None, **kw)
    if not defer:
        hook.defer_commit = False
    hm.register('k', hook)
    return hm, hook, DGDataLoader(dg, batch_size=bs, hook_manager=hm, output_pool=1)


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
def _order(mode):
    from tgm_amd import _native

    lib = _native.load()
    lib.tgmx_set_fused_order(mode)
    try:
        yield
    finally:
        lib.tgmx_set_fused_order(-1)  # back to TGMX_FUSED_ORDER / the library's default


def _fused(hook, batch):
    """Does the library plan this batch's shape as the fused launch?  (tgmx_recency_step_plan on a copy of the hook's argument block
    with the per-call fields the plan reads: the seed count and the hop outputs.)"""
    from tgm_amd import _native

    st = _native.RecencyStep()
    ctypes.memmove(ctypes.byref(st), ctypes.byref(hook._step), ctypes.sizeof(_native.RecencyStep))
    st.n_hops, st.n_groups, st.S0 = len(hook._num_nbrs), 0, batch.nbr_nids[0].shape[0]
    for h in range(st.n_hops):
        dense = not hook._by_id
        st.out_x[h] = batch.nbr_edge_x[h].data_ptr() if dense else None
        st.out_eid[h] = None if dense else batch.nbr_nids[h].data_ptr()  # (by id: the plan only asks whether edge ids go out)
    return bool(_native.load().tgmx_recency_step_plan(st) & 1)


def _lockstep(dg, N, ks, bs, keys=SRC_DST_NEG, reset_at=None, oracle=None, **kw):
    """Three pipelines, on orders 0, 1 and 2, batch by batch; `oracle(b, batch)` also checks order 2's batch b."""
    pipes = [_loader(dg, N, ks, bs, keys, **kw) for _ in range(3)]
    seen = 0
    with contextlib.ExitStack() as stack:
        for hm, _, _ in pipes:
            stack.enter_context(hm.activate('k'))
        its = [iter(p[2]) for p in pipes]
        b = 0
        while True:
            if reset_at is not None and b == reset_at:
                for _, h, _ in pipes:
                    h.reset_state()
            xs = []
            for mode, it in enumerate(its):
                with _order(mode):
                    xs.append(next(it, None))
            if xs[0] is None:
                assert xs[1] is None and xs[2] is None
                break
            assert all(_fused(p[1], x) for p, x in zip(pipes, xs)), 'the case does not reach the fused launch'
            for mode in (1, 2):
                _same(xs[0], xs[mode], f'order {mode} batch {b}')
            if oracle is not None:
                oracle(b, xs[2])
            seen += 1
            del xs
            b += 1
    for _, h, _ in pipes:
        h.check()
    if kw.get('mode', 'ring') == 'ring':
        for _, h, _ in pipes[1:]:
            assert torch.equal(pipes[0][1]._ring, h._ring), 'rings'
            assert torch.equal(pipes[0][1]._write_pos, h._write_pos), 'write_pos'
    assert seen >= 6
    return seen


@pytest.mark.parametrize('delta', ['1', '0'])
@pytest.mark.parametrize('defer', [True, False])
def test_wide_rows_three_groups(delta, defer, monkeypatch):
    """k = [20, 20], D = 172: one edge per batch (S0 = 3: fewer seeds than a workgroup has waves), seven (S0 = 21: workgroups straddle
    seeds and quads) and a hundred with hubs (several workgroups per quad pass, long rows next to pads)."""
    monkeypatch.setenv('TGMX_DELTA_WRITES', delta)
    _lockstep(_graph(*_stream(3, 10, 40, 172, 400)), 10, [20, 20], 1, defer=defer)
    _lockstep(_graph(*_stream(5, 30, 168, 172, 900)), 30, [20, 20], 7, defer=defer)
    _lockstep(_graph(*_stream(7, 300, 1000, 172, 3000, hubs=3)), 300, [20, 20], 100, defer=defer)


def test_quad_fallback_and_single_quad():
    # k0 = 5: no quads, mode 2 deals only; by id, the narrow rows take the fused launch too
    _lockstep(_graph(*_stream(11, 60, 400, 64, 2000)), 60, [5, 20], 20)
    _lockstep(_graph(*_stream(13, 60, 400, 6, 2000)), 60, [5, 5], 20, edge_features='by_id')
    # k0 = 4: C = 1, the quad pass is the whole launch
    _lockstep(_graph(*_stream(17, 60, 400, 5, 2000)), 60, [4, 64], 20)


def test_two_groups_and_one_group():
    _lockstep(_graph(*_stream(19, 80, 420, 172, 2000)), 80, [20, 20], 30, keys=SRC_DST)
    _lockstep(_graph(*_stream(23, 80, 420, 172, 2000)), 80, [20, 20], 30, keys=SRC)


def test_static_index():
    _lockstep(_graph(*_stream(29, 30, 168, 172, 900)), 30, [20, 20], 7, mode='csr')


def test_reset_in_the_middle():
    _lockstep(_graph(*_stream(31, 40, 210, 172, 900)), 40, [20, 20], 7, reset_at=11)


def test_by_id_features():
    _lockstep(_graph(*_stream(37, 100, 600, 172, 2000)), 100, [20, 20], 50, edge_features='by_id')


def test_against_the_cpu_ring_sampler():
    """Order 2 (dealt groups, quads; S0 = 14) against oracle/ring_port.py, batch by batch."""
    from oracle.ring_port import RingSamplerCPU

    N, E, D, bs, ks = 30, 168, 172, 7, [20, 20]
    src, dst, ts, x = _stream(41, N, E, D, 900)
    cpu = RingSamplerCPU(N, ks, D)

    def oracle(b, batch):
        lo, hi = b * bs, min((b + 1) * bs, E)
        hops = cpu.step(torch.cat([src[lo:hi], dst[lo:hi]]), torch.cat([ts[lo:hi], ts[lo:hi]]), src[lo:hi], dst[lo:hi], ts[lo:hi], x[lo:hi])
        for h, (_, _, o_i, o_t, o_x) in enumerate(hops):
            assert torch.equal(batch.nbr_nids[h].cpu(), o_i), f'ids differ (batch {b}, hop {h})'
            assert torch.equal(batch.nbr_edge_time[h].cpu(), o_t), f'times differ (batch {b}, hop {h})'
            assert torch.equal(batch.nbr_edge_x[h].cpu(), o_x), f'feats differ (batch {b}, hop {h})'

    _lockstep(_graph(src, dst, ts, x), N, ks, bs, keys=SRC_DST, oracle=oracle)
