"""The fused hop-0 + hop-1 launch reads a row's old span (out_valid: what the row still holds from the previous call) at the top of
its wave, ahead of the seed -> pick -> gather chain.  The spans are state carried from call to call on a pool of one, so every case
runs consecutive batches through one output set and checks each against the CPU ring sampler (oracle/ring_port.py), bit for bit:
a stale or misplaced span shows as a feature row that kept old contents or lost its zeros."""

import ctypes

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
    x = torch.rand((E, D), generator=g)
    return src, dst, ts, x


def _fused(hook, batch):
    """Does the library plan this batch's shape as the fused launch?  (tgmx_recency_step_plan on a copy of the hook's argument block
    with the per-call fields the plan reads: the seed count and the hop outputs.)"""
    from tgm_amd import _native

    st = _native.RecencyStep()
    ctypes.memmove(ctypes.byref(st), ctypes.byref(hook._step), ctypes.sizeof(_native.RecencyStep))
    st.n_hops, st.n_groups, st.S0 = len(hook._num_nbrs), 0, batch.nbr_nids[0].shape[0]
    for h in range(st.n_hops):
        st.out_x[h] = batch.nbr_edge_x[h].data_ptr()
    return bool(_native.load().tgmx_recency_step_plan(st) & 1)


def _run(seed, N, E, D, ks, bs, tmax, hubs=0, defer=True, one_group=False):
    """One pipeline over the stream, every batch against the CPU sampler fed the same seeds."""
    from oracle.ring_port import RingSamplerCPU
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import HookManager, RecencyNeighborHook

    src, dst, ts, x = _stream(seed, N, E, D, tmax, hubs)
    dg = DGraph(DGData.from_raw(ts, torch.stack([src, dst], 1), x), device=DEV)
    keys = (['edge_src'], ['edge_time']) if one_group else (['edge_src', 'edge_dst'], ['edge_time', 'edge_time'])
    hook = RecencyNeighborHook(N, ks, keys[0], keys[1], validate='deferred')
    if not defer:
        hook.defer_commit = False
    hm = HookManager(keys=['k'])
    hm.register('k', hook)
    cpu = RingSamplerCPU(N, ks, D)
    seen = 0
    with hm.activate('k'):
        for b, batch in enumerate(DGDataLoader(dg, batch_size=bs, hook_manager=hm, output_pool=1)):
            lo, hi = b * bs, min((b + 1) * bs, E)
            seeds = src[lo:hi] if one_group else torch.cat([src[lo:hi], dst[lo:hi]])
            times = ts[lo:hi] if one_group else torch.cat([ts[lo:hi], ts[lo:hi]])
            hops = cpu.step(seeds, times, src[lo:hi], dst[lo:hi], ts[lo:hi], x[lo:hi])
            assert _fused(hook, batch), 'the case does not reach the fused launch'
            for h, (_, _, o_i, o_t, o_x) in enumerate(hops):
                assert torch.equal(batch.nbr_nids[h].cpu(), o_i), f'ids differ (batch {b}, hop {h})'
                assert torch.equal(batch.nbr_edge_time[h].cpu(), o_t), f'times differ (batch {b}, hop {h})'
                assert torch.equal(batch.nbr_edge_x[h].cpu(), o_x), f'feats differ (batch {b}, hop {h})'
            seen += 1
    hook.check()
    assert seen >= 6


@pytest.mark.parametrize('delta', ['1', '0'])
@pytest.mark.parametrize('defer', [True, False])
def test_wide_rows(delta, defer, monkeypatch):
    """k = [20, 20], D = 172: one edge per batch (fewer seeds than a workgroup has waves: hop-0 and hop-1 waves share workgroups),
    seven (workgroups straddle seeds) and a hundred with hubs (full rows next to pads, rows that shrink and grow between calls)."""
    monkeypatch.setenv('TGMX_DELTA_WRITES', delta)
    _run(3, 10, 40, 172, [20, 20], 1, 400, defer=defer)
    _run(5, 30, 168, 172, [20, 20], 7, 900, defer=defer)
    _run(7, 300, 1000, 172, [20, 20], 100, 3000, hubs=3, defer=defer)


def test_other_row_shapes_and_one_seed_group():
    _run(11, 60, 400, 64, [5, 20], 20, 2000)  # k0 = 5: hop-1 rows of a seed straddle workgroups unevenly
    _run(17, 60, 400, 5, [4, 64], 20, 2000)   # one workgroup per seed, 64-slot rows of single floats
    _run(23, 80, 420, 172, [20, 20], 30, 2000, one_group=True)
