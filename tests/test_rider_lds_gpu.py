"""The ring-update rider of the fused hop-0 + hop-1 launch at m <= 512 entries (kSideAll: one workgroup sorts the batch in LDS and
decides its placement) at its edges: one entry per half, the 256-entry chunk boundary, the plan's 512-entry limit and the first
size past it, time ties, runs longer than B, the int32 key wrap.  Every batch's outputs, and the ring state at the end, are compared
bit for bit with the CPU restatement of the reference (oracle.ring_port.RingSamplerCPU), fed the batch's own hop-0 seeds."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
D, KS = 64, [10, 10]  # rows wide enough for the fused plan (the packed narrow-row kernel does not take them)


def _stream(seed, N, E, tmax, hubs=0, tlo=1):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    if hubs:  # most edges touch one of `hubs` nodes, a third of those on BOTH ends
        pick = torch.rand((E,), generator=g) < 0.7
        dst = torch.where(pick, torch.randint(0, hubs, (E,), generator=g, dtype=torch.int32), dst)
        both = pick & (torch.rand((E,), generator=g) < 0.33)
        src = torch.where(both, dst, src)
    ts = torch.sort(torch.randint(tlo, tmax, (E,), generator=g, dtype=torch.int64)).values
    x = torch.rand((E, D), generator=g)
    return src, dst, ts, x


def _pipeline(st, N, bs, defer=True, directed=False, key_arith='int32'):
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook

    src, dst, ts, x = st
    dg = DGraph(DGData.from_raw(ts, torch.stack([src, dst], 1), x), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(0, N, seed=5))
    hook = RecencyNeighborHook(N, KS, ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time'], mode='ring', validate='deferred',
                               directed=directed, key_arith=key_arith)
    hook.defer_commit = defer
    hm.register('k', hook)
    return hm, hook, DGDataLoader(dg, batch_size=bs, hook_manager=hm, output_pool=1)


def _against_oracle(st, N, bs, n_batches, defer=True, directed=False, key_arith='int32'):
    from oracle.ring_port import RingSamplerCPU

    src, dst, ts, x = st
    E = src.numel()
    n_batches = min(n_batches, (E + bs - 1) // bs)
    hm, hook, loader = _pipeline(st, N, bs, defer, directed, key_arith)
    ref = RingSamplerCPU(N, KS, D, directed, key_arith=key_arith)
    seen = 0
    with hm.activate('k'):
        for b, batch in enumerate(loader):
            if b == n_batches:
                break
            lo, hi = b * bs, min((b + 1) * bs, E)
            hops = ref.step(batch.seed_nids[0].cpu(), batch.seed_times[0].cpu(), src[lo:hi], dst[lo:hi], ts[lo:hi], x[lo:hi])
            for h, (_, _, o_i, o_t, o_x) in enumerate(hops):
                assert torch.equal(batch.nbr_nids[h].cpu(), o_i), f'batch {b} hop {h} ids'
                assert torch.equal(batch.nbr_edge_time[h].cpu(), o_t), f'batch {b} hop {h} times'
                assert torch.equal(batch.nbr_edge_x[h].cpu(), o_x), f'batch {b} hop {h} features'
            seen += 1
            del batch
    hook.check()
    assert seen == n_batches
    # the state after the last batch (the properties flush a pending commit)
    B = max(KS)
    ring = hook._ring.cpu().view(torch.int32).reshape(N, B, 4)
    live = ref.ids >= 0
    assert torch.equal(ring[:, :, 0], ref.ids), 'ring ids'
    rt = ring[:, :, 2:4].contiguous().view(torch.int64).view(N, B)
    assert torch.equal(rt[live], ref.times[live]), 'ring times'
    assert torch.equal(hook._ring_x.cpu().reshape(N, B, D)[live], ref.feats[live]), 'ring_x of live slots'
    assert torch.equal(hook._write_pos.cpu().long(), ref.wpos), 'write_pos'


# m = 2 bs: 2, 254, 256 (one chunk, full), 258 (the second chunk holds two entries), 400 (the headline), 510, 512 (both chunks full);
# bs = 257: m = 514 takes the plan of a rider per chunk, unchanged
@pytest.mark.parametrize('bs', [1, 127, 128, 129, 200, 255, 256, 257])
def test_sizes_undirected(bs):
    n_batches = 40 if bs == 1 else 30
    _against_oracle(_stream(100 + bs, 700, n_batches * bs + bs // 2, 60_000), 700, bs, n_batches + 1)


@pytest.mark.parametrize('bs', [511, 512])
def test_sizes_directed(bs):
    _against_oracle(_stream(300 + bs, 900, 30 * bs + 77, 80_000), 900, bs, 31, directed=True)


@pytest.mark.parametrize('bs', [129, 200, 256])
def test_time_ties_and_long_runs(bs):
    """tmax so small that a batch holds few distinct timestamps (the tie order is the entry index), and hubs on both ends of many
    edges of a batch: runs longer than B = 10, several runs of one node colliding on its slots."""
    _against_oracle(_stream(500 + bs, 60, 31 * bs, 40, hubs=3), 60, bs, 31)


@pytest.mark.parametrize('key_arith', ['int32', 'int64'])
@pytest.mark.parametrize('bs', [200, 256])
def test_key_wrap(bs, key_arith):
    """node * span wraps in int32 (N = 3000, timestamps near 10^6): a node's entries split into several runs of the sorted order."""
    _against_oracle(_stream(700 + bs, 3000, 31 * bs, 1_000_000, tlo=900_000), 3000, bs, 31, key_arith=key_arith)


@pytest.mark.parametrize('bs', [129, 256])
def test_without_deferral(bs):
    """defer_commit = False: the commit launch behind the lookups reads the rider's scratch arrays."""
    _against_oracle(_stream(900 + bs, 500, 31 * bs, 30_000, hubs=2), 500, bs, 31, defer=False)
