"""BatchAnalyticsHook, EdgeEventsSeenNodesTrackHook and NodeAnalyticsHook on the device (csrc/analytics.hip), DeviceTransferHook and
PinMemoryHook with one: the g27 / g28 / g29 fixtures, and the device path against the host path -- which states the definitions in Python over
sets -- on streams at the kernels' dispatch edges.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import analytics_cases as ac
from tgm_amd import DGData, DGDataLoader, DGraph
from tgm_amd.hooks import BatchAnalyticsHook, DeviceTransferHook, EdgeEventsSeenNodesTrackHook, HookManager, NodeAnalyticsHook, PinMemoryHook

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 700  # nodes of the generated streams
TRACKED = {1: [321], 64: list(range(3, 3 + 64 * 7, 7)), 65: list(range(5, 5 + 65 * 9, 9)), N: list(range(N))}


@pytest.mark.parametrize('name', ac.fixtures('g27_batch_analytics'))
def test_batch_analytics_fixture(name):
    assert ac.replay_batch_analytics(name, DEV) == ac.replay_batch_analytics(name, 'cpu')


@pytest.mark.parametrize('name', ac.fixtures('g28_seen_nodes'))
def test_seen_nodes_fixture(name):
    (hook, on_dev), (host, on_host) = ac.replay_seen_nodes(name, DEV), ac.replay_seen_nodes(name, 'cpu')
    ac.assert_same_seen(on_dev, on_host, name)
    assert hook._seen_mask.device.type == 'cuda' and torch.equal(hook._seen_mask.cpu(), host._seen_mask)
    hook.check()


@pytest.mark.parametrize('name', ac.fixtures('g29_node_analytics'))
def test_node_analytics_fixture(name):
    (hook, on_dev), (host, on_host) = ac.replay_node_analytics(name, DEV), ac.replay_node_analytics(name, 'cpu')
    ac.assert_same_node_runs(on_dev, on_host, name)
    assert hook.state() == host.state()
    hook.check()


@pytest.mark.parametrize('ids', [np.int32, np.int64])
def test_batch_analytics_device_equals_host(ids):
    batches = ac.sized_batches(2720, N, ids=ids)
    on_dev, on_host = ac.run_batch_analytics(batches, DEV), ac.run_batch_analytics(batches, 'cpu')
    for i, (d, h) in enumerate(zip(on_dev, on_host)):
        assert d == h, f'batch {i} (E {len(batches[i]["edge_src"])}, Nn {len(batches[i]["node_x_nids"])}): {d} != {h}'
    assert any(v[5] > 0 for v in on_host) and any(v[6] > 0 for v in on_host)  # the streams do repeat events


@pytest.mark.parametrize('ids', [np.int32, np.int64])
def test_seen_nodes_device_equals_host(ids):
    batches = ac.sized_batches(2820, N, ids=ids, labels=True)
    (hook, on_dev), (host, on_host) = ac.run_seen_nodes(N, batches, DEV), ac.run_seen_nodes(N, batches, 'cpu')
    ac.assert_same_seen(on_dev, on_host, str(ids))
    assert torch.equal(hook._seen_mask.cpu(), host._seen_mask)
    assert 0 < len(on_host[2][0]) < len(batches[2]['node_y_nids'])  # some labelled nodes seen, some not
    hook.check()


@pytest.mark.parametrize('ids', [np.int32, np.int64])
@pytest.mark.parametrize('T', sorted(TRACKED))
def test_node_analytics_device_equals_host(T, ids):
    batches = ac.sized_batches(2920 + T, N, ids=ids)
    (hook, on_dev), (host, on_host) = ac.run_node_analytics(TRACKED[T], N, batches, DEV), ac.run_node_analytics(TRACKED[T], N, batches, 'cpu')
    ac.assert_same_node_runs(on_dev, on_host, f'T {T}')
    assert hook.state() == host.state()
    hook.check()


def test_node_analytics_tables_rehash():
    """16 slots to begin with: every table has to grow, more than once, and nothing is lost on the way"""
    batches = ac.sized_batches(2930, N)[2:6] + ac.sized_batches(2931, N)[2:6]
    hook, on_dev = ac.run_node_analytics(TRACKED[65], N, batches, DEV, capacity=16)
    host, on_host = ac.run_node_analytics(TRACKED[65], N, batches, 'cpu')
    assert hook.rehashes >= 2, hook.rehashes
    ac.assert_same_node_runs(on_dev, on_host, 'rehash')
    assert hook.state() == host.state()
    hook.check()


def test_batch_analytics_without_sync_reads_nothing_back():
    """sync=False under torch's sync debug mode (any synchronising call raises); the tensors hold sync=True's values bit for bit"""
    batches = ac.sized_batches(2730, N)[1:8]
    on_dev = [ac.batch_of(b, DEV) for b in batches]
    want = ac.run_batch_analytics(batches, DEV)
    hook, dg = BatchAnalyticsHook(sync=False), ac.dg_on(DEV)
    hook(dg, ac.batch_of(batches[0], DEV))  # the library's first load and the workspace query are not the path
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = [ac.batch_analytics_values(hook(dg, b)) for b in on_dev]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for g, w in zip(got, want):
        assert all(v.dim() == 0 and v.device.type == 'cuda' and v.dtype == (torch.float32 if k == 'avg_degree' else torch.int64) for k, v in zip(ac.BA_KEYS, g))
        assert len({v.untyped_storage().data_ptr() for v in g}) == 1  # views of one buffer
        assert [v.item() for v in g] == w
        assert np.float32(g[4].item()).tobytes() == np.float32(w[4]).tobytes()


def test_seen_nodes_ids_outside_set_the_status():
    good = [ac.B([1, 2], [3, 4], y=[1, 9, 3]), ac.B([5], [6], y=[7, 5, 1, 8, 6, 2])]
    bad = [good[0], ac.B([5, 10, 2**31 - 1, -1], [6, 3, 0, 4], y=[7, 5, 1, 10, 8, 6, -3, 2])]  # the edges and labels of `good`, and ids outside [0, 10) among them
    hook, on_dev = ac.run_seen_nodes(10, bad[:1], DEV)
    hook.check()
    _, more = ac.run_seen_nodes(10, bad[1:], DEV, hook=hook)
    host, on_host = ac.run_seen_nodes(10, good, 'cpu')
    # the in-range part: the edges (10, 3) and (2^31 - 1, 0) and (-1, 4) still mark 3, 0, 4 -- ids are marked one by one
    host._seen_mask[torch.tensor([3, 0, 4])] = True
    assert more[0][0].tolist() == [5, 1, 6, 2] and more[0][1].tolist() == [1, 2, 5, 7]
    assert torch.equal(hook._seen_mask.cpu(), host._seen_mask)
    with pytest.raises(ValueError, match=r'ids must lie in \[0, 10\)'):
        hook.check()
    hook.check()  # reported once


def test_node_analytics_events_outside_take_no_part():
    """an event with an id outside [0, num_nodes) or a negative time: the rest of the batch is answered as if it were not there, check()
    reports it once, the state does not hold it"""
    first = ac.B([0, 1], [1, 2], [3, 4], [2], [4])
    good = ac.B([0, 3, 1], [2, 0, 1], [5, 6, 7], [1, 4], [7, 7])
    with_bad = ac.B([0, 6, 3, 1, 2, 1], [2, 0, 0, 2**31 - 1, -1, 1], [5, 5, 6, 9, 9, 7], [1, 6, 4, -2], [7, 8, 7, 8])
    negative_time = ac.B([0, 3, 2, 1], [2, 0, 3, 1], [5, 6, -1, 7], [1, 0, 4], [7, -4, 7])
    host, on_host = ac.run_node_analytics([0, 1, 4], 6, [first, good], 'cpu')
    for bad_batch, message in ((with_bad, 'ids must lie'), (negative_time, 'times >= 0')):
        hook, on_dev = ac.run_node_analytics([0, 1, 4], 6, [first], DEV)
        hook.check()
        _, more = ac.run_node_analytics([0, 1, 4], 6, [bad_batch], DEV, hook=hook)
        ac.assert_same_node_runs(on_dev + more, on_host, message)
        assert hook.state() == host.state()
        with pytest.raises(ValueError, match=message):
            hook.check()
        hook.check()  # reported once


def test_a_field_left_on_the_host_is_refused():
    """the kernels take raw pointers: a batch with one field on another device raises before anything is launched"""
    fields = ac.B([0, 1], [1, 2], [3, 4], [2], [4], y=[1, 2])
    hooks = (BatchAnalyticsHook(), NodeAnalyticsHook(torch.tensor([0, 1]), 6), EdgeEventsSeenNodesTrackHook(6))
    for hook, stray in zip(hooks, ('edge_dst', 'node_x_time', 'node_y_nids')):
        batch = ac.batch_of(fields, DEV)
        setattr(batch, stray, getattr(batch, stray).cpu())
        with pytest.raises(ValueError, match=f'{stray} is on cpu'):
            hook(ac.dg_on(DEV), batch)
    assert hooks[1].state()['edges'] == set() and not hooks[2]._seen_mask.any()


def test_seen_nodes_strided_fields():
    """every second element of longer tensors: read as the values they show, not as the memory under them"""
    b = ac.B([1, 9, 2, 9], [3, 9, 4, 9], y=[3, 8, 5, 8, 1, 8])
    strided = ac.batch_of(b, DEV)
    for k in ('edge_src', 'edge_dst', 'node_y_nids'):
        setattr(strided, k, getattr(strided, k)[::2])
        assert not getattr(strided, k).is_contiguous()
    hook = EdgeEventsSeenNodesTrackHook(10)
    out = hook(ac.dg_on(DEV), strided)
    assert out.seen_nodes.tolist() == [3, 1] and out.batch_nodes_mask.tolist() == [0, 2] and out.seen_nodes.dtype == torch.int32
    assert hook._seen_mask.nonzero().view(-1).tolist() == [1, 2, 3, 4]
    hook.check()


def test_reset_state_on_the_device():
    batches = ac.sized_batches(2940, N, labels=True)[1:5]
    hook, _ = ac.run_node_analytics(TRACKED[64], N, batches, DEV)
    hook.reset_state()
    assert hook.state() == dict(first={}, last={}, appearances={}, edges=set(), nbrs=set(), times=set(), apps=set())
    _, again = ac.run_node_analytics(TRACKED[64], N, batches, DEV, hook=hook)
    fresh, want = ac.run_node_analytics(TRACKED[64], N, batches, DEV)
    ac.assert_same_node_runs(again, want, 'after reset')
    assert hook.state() == fresh.state()
    seen, _ = ac.run_seen_nodes(N, batches, DEV)
    _, again = ac.run_seen_nodes(N, ['reset'] + batches, DEV, hook=seen)
    ac.assert_same_seen(again, ac.run_seen_nodes(N, batches, DEV)[1], 'after reset')


def labelled_graph(device):
    rng = np.random.default_rng(2950)
    E, Ny, n = 600, 240, 80
    t = np.sort(rng.integers(0, 3000, E))
    ei = torch.tensor(np.stack([rng.integers(0, n // 2, E), rng.integers(0, n, E)], 1).astype(np.int32))
    ty = np.sort(rng.integers(0, 3000, Ny))
    data = DGData.from_raw(torch.tensor(t), ei, node_y_time=torch.tensor(ty), node_y_nids=torch.tensor(rng.integers(0, n, Ny).astype(np.int32)),
                           node_y=torch.tensor(rng.random((Ny, 3), dtype=np.float32)))  # fmt: skip
    return DGraph(data, device=device), n


@pytest.mark.parametrize('hook_id', [None, 'foo'])
def test_through_loader_and_hook_manager(hook_id):
    """the nodeproppred pattern: z[batch.seen_nodes] against y[batch.batch_nodes_mask], device loader against host loader"""
    sfx = f'_{hook_id}' if hook_id else ''

    def run(device):
        dg, n = labelled_graph(device)
        hm = HookManager(keys=['train'])
        hooks = (EdgeEventsSeenNodesTrackHook(n, id=hook_id), BatchAnalyticsHook(id=hook_id), NodeAnalyticsHook(torch.arange(0, n, 3), n, id=hook_id))
        for h in hooks:
            hm.register('train', h)
        z, out = torch.arange(n * 2, dtype=torch.float32, device=device).view(n, 2), []
        with hm.activate('train'):
            for batch in DGDataLoader(dg, batch_size=100, hook_manager=hm):
                seen, pos = getattr(batch, 'seen_nodes' + sfx), getattr(batch, 'batch_nodes_mask' + sfx)
                assert (hook_id is None) == hasattr(batch, 'seen_nodes')
                if batch.node_y is not None and len(seen):
                    z_node, y = z[seen], batch.node_y[pos]
                    assert z_node.shape[0] == y.shape[0] and torch.equal(batch.node_y_nids[pos], seen)
                out.append((seen.cpu(), pos.cpu(), ac.batch_analytics_values(batch, sfx), getattr(batch, 'node_stats' + sfx), getattr(batch, 'edge_stats' + sfx)))
        for h in hooks[::2]:
            h.check()
        return out

    on_dev, on_host = run(DEV), run('cpu')
    assert len(on_dev) == len(on_host) == 9 and sum(len(o[0]) for o in on_host) > 0  # 600 edges + 240 labels, 100 events a batch
    for i, (d, h) in enumerate(zip(on_dev, on_host)):
        assert torch.equal(d[0], h[0]) and torch.equal(d[1], h[1]) and d[2:] == h[2:], f'batch {i}'


def test_device_transfer_and_pin_memory():
    host, _ = labelled_graph('cpu')
    batch = host.materialize()
    batch.foo, batch.bar = torch.rand(1, 2), [torch.rand(3), ('a', torch.rand(2))]
    assert PinMemoryHook()(host, batch) is batch
    assert batch.edge_src.is_pinned() and batch.edge_time.is_pinned() and batch.foo.is_pinned() and batch.bar[1][1].is_pinned()
    pinned = batch.edge_src
    assert PinMemoryHook()(host, batch).edge_src is pinned  # already pinned: by identity
    hook = DeviceTransferHook('cuda')
    assert hook(host, batch) is batch
    torch.cuda.synchronize()
    moved = [batch.edge_src, batch.edge_dst, batch.edge_time, batch.node_y, batch.foo, batch.bar[0], batch.bar[1][1]]
    assert all(t.device.type == 'cuda' for t in moved) and batch.bar[1][0] == 'a'
    assert torch.equal(batch.edge_src.cpu(), pinned)
    src = batch.edge_src
    assert hook(host, batch) is batch and batch.edge_src is src  # already there: by identity
    dev, _ = labelled_graph(DEV)
    batch = dev.materialize()
    src = batch.edge_src
    assert src.device.type == 'cuda' and hook(dev, batch) is batch and batch.edge_src is src
    assert PinMemoryHook()(dev, batch) is batch and batch.edge_src is src
