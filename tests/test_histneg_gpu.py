"""HistoricalNegativeEdgeSamplerHook on the device (csrc/histneg.hip): the g25 fixtures, and the device path against the host path bit for bit
-- the host path states the draw in Python over per-source lists, so equal ids mean the chains hold every source's events in arrival order."""
import numpy as np
import pytest
import torch

import histneg_cases as hc
from tgm_amd import DGDataLoader
from tgm_amd.hooks import HistoricalNegativeEdgeSamplerHook, HookManager, RecencyNeighborHook

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STREAMS = hc.extra_streams()


@pytest.mark.parametrize('name', hc.FIXTURES)
def test_fixture_on_the_device_and_against_the_host_path(name):
    hook, on_dev = hc.replay(name, DEV, seed=5)
    host, on_host = hc.replay(name, 'cpu', seed=5)
    hc.assert_same_runs(on_dev, on_host, name)
    assert hook.histories() == host.histories()
    hook.check()


@pytest.mark.parametrize('name', [n for n in STREAMS if n != 'one_per_call'])
def test_device_equals_host_path(name):
    calls, kw = STREAMS[name]
    hook, on_dev = hc.run_stream(calls, DEV, **kw)
    host, on_host = hc.run_stream(calls, 'cpu', **kw)
    hc.assert_same_runs(on_dev, on_host, name)
    assert hook.histories() == host.histories()
    hook.check()
    if name == 'reallocating':
        caps = sorted({o[2].shape[1] for o in on_dev})
        assert hook.pool_grown >= 2 and len(caps) >= 3, (hook.pool_grown, caps)
    if name == 'skewed_256':  # 256 events of a new source in one batch: the segments 0..6, filled in batch order
        assert hook.histories()[3][:256] == list(range(1000, 1256)) and on_dev[1][0].tolist()[1] == -1


def test_every_rank_is_drawn():
    """a source grown to 29 events one call at a time (past the segment boundaries 4, 12 and 28), then drawn: over the seeds every one of the 29
    ranks comes back, and each time it is the host path's"""
    calls, _ = STREAMS['one_per_call']
    dg_dev, dg_host = hc.stream_graph(calls, DEV), hc.stream_graph(calls, 'cpu')
    seen = set()
    for seed in range(96):  # (the 89th seed brings the last rank)
        _, on_dev = hc.run_stream(calls, DEV, seed=seed, dg=dg_dev)
        if seed < 8:  # whole runs (every intermediate history length) for a few seeds, the final draw for all
            hc.assert_same_runs(on_dev, hc.run_stream(calls, 'cpu', seed=seed, dg=dg_host)[1], f'seed {seed}')
        last = int(on_dev[-1][0][0])
        assert last == 100 + hc.historical_draw(seed, 30, 4, 29)
        seen.add(last - 100)
    assert seen == set(range(29))


def test_out_of_range_source_sets_the_status():
    calls = [([1, 2, 1], [5, 6, 7], [0, 1, 2]), ([1, 2, 9], [3, 3, 3], [3, 4, 5])]
    dg = hc.stream_graph(calls, DEV)
    N = dg._storage.num_nodes_global
    hook = HistoricalNegativeEdgeSamplerHook(seed=1)
    hook(dg, hc.batch_of(*calls[0], dg.device))
    hook.check()
    b = hook(dg, hc.batch_of([1, N, 2, 2**31 - 1, N + 7], [8, 8, 8, 8, 8], [3, 3, 3, 3, 3], dg.device))
    neg = b.neg.tolist()
    assert neg[0] in (5, 7) and neg[2] == 6 and neg[1] == neg[3] == neg[4] == -1
    assert b.valid_neg_mask.tolist() == [True, False, True, False, False]
    with pytest.raises(ValueError, match='source ids'):
        hook.check()
    hook.check()  # reported once
    assert hook.histories() == {1: [5, 7, 8], 2: [6, 8]}  # the ids outside joined no history; the log keeps them, as the reference's would
    assert hook._memory[0, :8].tolist() == [1, 2, 1, 1, N, 2, 2**31 - 1, N + 7]


def test_a_batch_reads_nothing_back():
    """batches, among them ones that make the host grow the pool and the log, under torch's sync debug mode: any synchronising call raises"""
    calls, _ = STREAMS['reallocating']
    calls = calls[:12]
    dg = hc.stream_graph(calls, DEV)
    batches = [hc.batch_of(*c, dg.device) for c in calls]

    def run(guard):
        hook = HistoricalNegativeEdgeSamplerHook(seed=11, _initial_pool_words=8)
        hook(dg, batches[0])  # the library's first load and the workspace query are not the path
        torch.cuda.synchronize()
        if guard:
            torch.cuda.set_sync_debug_mode('error')
        try:
            out = [hook(dg, b).neg for b in batches[1:]]
        finally:
            torch.cuda.set_sync_debug_mode('default')
        hook.check()
        return hook, torch.cat(out).cpu()

    (h0, n0), (h1, n1) = run(True), run(False)
    assert h0.pool_grown >= 2 and h0._count == 12 * 64
    # two runs export identical state
    assert torch.equal(n0, n1) and h0.histories() == h1.histories() and torch.equal(h0._memory, h1._memory)
    assert torch.equal(n0, torch.cat([o[0] for o in hc.run_stream(calls, 'cpu', seed=11)[1][1:]]))


@pytest.mark.parametrize('hook_id', [None, 'foo'])
def test_through_loader_and_hook_manager(hook_id):
    calls = hc.fixture_calls('g25_histneg_wiki_small')[2]
    dg = hc.stream_graph(calls, DEV)
    hm = HookManager(keys=['train'])
    hook = HistoricalNegativeEdgeSamplerHook(id=hook_id, seed=21)
    hm.register('train', hook)
    by_hand = hc.run_stream(calls, DEV, seed=21, dg=dg)[1]
    suffix = f'_{hook_id}' if hook_id else ''
    with hm.activate('train'):
        n = 0
        for batch, (neg, mask, _, _), (_, _, t) in zip(DGDataLoader(dg, batch_size=200, hook_manager=hm), by_hand, calls):
            assert torch.equal(getattr(batch, 'neg' + suffix).cpu(), neg) and torch.equal(getattr(batch, 'valid_neg_mask' + suffix).cpu(), mask)
            assert torch.equal(getattr(batch, 'neg_time' + suffix).cpu(), torch.tensor(t))
            assert (hook_id is None) == hasattr(batch, 'neg')
            n += 1
    assert n == 10 and hook._count == 2000
    hook.check()


def test_not_lowered_into_the_fused_pipeline():
    """a manager whose first hook is this one runs hook by hook"""
    from tgm_amd.pipeline import CompiledPipeline

    calls = hc.fixture_calls('g25_histneg_mixed')[2]
    dg = hc.stream_graph(calls, DEV)
    hooks = [HistoricalNegativeEdgeSamplerHook(), RecencyNeighborHook(dg._storage.num_nodes_global, [2], ['edge_src', 'edge_dst'], ['edge_time', 'edge_time'])]
    assert CompiledPipeline.lower(dg, hooks, None) is None
