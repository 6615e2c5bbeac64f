"""NeighborSamplerHook past 64 neighbours per hop (``tgmx_uniform_lookup_wide``): the kernel against the serial shuffle that defines the draw
(the same loop pins the k <= 64 kernel at k = 64: one definition), and the hook against the reference restatement where that is deterministic."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0) if torch.cuda.is_available() else None
M64 = (1 << 64) - 1
N, E, HUB = 8, 50_010, 0  # edge e is hub - (1 + e % 5), undirected: the hub has ev_hi candidates, nodes 1..5 a fifth each, 6 and 7 none
RNG_SEED, RNG_STREAM = 0x1234_5678_9ABC_DEF1, (7 << 8) | 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(n, c, k):
    """Candidate index behind every valid output slot of node n: the definition, a serial loop over a dict of overrides."""
    if c <= k:
        return list(range(c))
    base = splitmix64(RNG_SEED ^ splitmix64(RNG_STREAM ^ ((n & 0xFFFFFFFF) << 32)))
    a, out = {}, []
    for i in range(k):
        j = i + ((splitmix64((base + i) & M64) * (c - i)) >> 64)
        out.append(a.get(j, j))
        a[j] = a.get(i, i)
    return out


@functools.lru_cache(maxsize=None)
def _graph(D):
    from tgm_amd.index import build_csr

    src, dst, ts = np.full(E, HUB, np.int32), (1 + np.arange(E) % 5).astype(np.int32), 10 + 3 * np.arange(E, dtype=np.int64)
    x = np.random.default_rng(D).random((E, D), dtype=np.float32)
    csr = build_csr(*(torch.from_numpy(v).to(DEV) for v in (src, dst, ts)), N, order='event', directed=False)
    return src, dst, ts, x, csr, torch.from_numpy(x).to(DEV)


def _lookup(k, D, ev_hi, seeds):
    from tgm_amd import _native

    csr, x_dev = _graph(D)[4:]
    fn = getattr(_native.load(), 'tgmx_uniform_lookup_csr' if k <= 64 else 'tgmx_uniform_lookup_wide')
    S, seeds_dev = len(seeds), torch.tensor(seeds, dtype=torch.int32, device=DEV)
    nid, nts = (torch.full((S, k), -7, dtype=t, device=DEV) for t in (torch.int32, torch.int64))
    nx, status = torch.full((S, k, D), -7.0, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = fn(csr.indptr.data_ptr(), csr.adj.data_ptr(), x_dev.data_ptr() if D else None, D, seeds_dev.data_ptr(), S, k, ev_hi, N, 1, RNG_SEED, RNG_STREAM,
            nid.data_ptr(), nts.data_ptr(), nx.data_ptr() if D else None, status.data_ptr(), _native.stream_ptr(0))  # fmt: skip
    _native.check(rc, fn.__name__)
    return nid.cpu().numpy(), nts.cpu().numpy(), nx.cpu().numpy(), int(status.item())


@pytest.mark.parametrize('D', [0, 5, 8, 65, 130])  # 8: rows move in 16-byte pieces; 130: more than one trip per row
@pytest.mark.parametrize('c_of_k', [lambda k: 0, lambda k: k - 1, lambda k: k, lambda k: k + 1, lambda k: 2 * k + 3, lambda k: 50_000],
                         ids=['c0', 'k-1', 'k', 'k+1', '2k+3', '50000'])  # fmt: skip
@pytest.mark.parametrize('k', [64, 65, 128, 200, 2048])
def test_wide_kernel_is_the_serial_shuffle(k, c_of_k, D):
    """ev_hi cuts the hub's row after c of its 50 010 entries.  Seeds: the hub twice (equal rows), a node with a fifth of the hub's
    candidates, a -1 (allow_pad: all pads, status clean) and a node without edges; then an id >= N on its own (status set, all pads)."""
    ev_hi = c_of_k(k)
    src, dst, ts, x = _graph(D)[:4]
    seeds = [HUB, 3, HUB, -1, 6]
    e_n, e_t, e_x = np.full((5, k), -1, np.int32), np.zeros((5, k), np.int64), np.zeros((5, k, D), np.float32)
    for r, n in enumerate(seeds):
        if n >= 0:
            cand = np.nonzero((src[:ev_hi] == n) | (dst[:ev_hi] == n))[0]  # (eid, role) order; no self loops: one entry per edge
            eids = cand[np.asarray(draw(n, len(cand), k), np.int64)]
            e_n[r, : len(eids)] = np.where(src[eids] == n, dst[eids], src[eids])
            e_t[r, : len(eids)], e_x[r, : len(eids)] = ts[eids], x[eids]
    g_n, g_t, g_x, status = _lookup(k, D, ev_hi, seeds)
    assert status == 0
    assert np.array_equal(g_n, e_n) and np.array_equal(g_t, e_t) and g_x.tobytes() == e_x.tobytes()
    assert np.array_equal(g_n[0], g_n[2]) and np.array_equal(g_t[0], g_t[2])
    assert ev_hi <= k or len(set(g_t[0].tolist())) == k  # a sampled row: k distinct candidates
    b_n, b_t, b_x, status = _lookup(k, D, ev_hi, [N + 2])
    assert status == 1  # TGMX_ST_SEED_RANGE
    assert (b_n == -1).all() and (b_t == 0).all() and (b_x == 0).all()


@pytest.mark.parametrize('ks', [[80], [70, 66]], ids=str)
def test_hook_past_64_neighbours(ks):
    from oracle import uniform_ref
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import HookManager, NeighborSamplerHook

    rng = np.random.default_rng(11)
    n_nodes, n_edges, D, bs = 30, 400, 3, 100
    src, dst = (rng.integers(0, n_nodes, n_edges).astype(np.int32) for _ in range(2))
    src[::2] = 0  # a hub: past 80 candidates from the third batch on, so both kinds of row occur
    ts = np.sort(rng.integers(1, 200, n_edges)).astype(np.int64)
    edge_x = rng.random((n_edges, D), dtype=np.float32)
    dg = DGraph(DGData.from_raw(torch.from_numpy(ts), torch.stack([torch.from_numpy(src), torch.from_numpy(dst)], 1), torch.from_numpy(edge_x)), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', NeighborSamplerHook(ks, ['edge_src', 'edge_dst'], ['edge_time', 'edge_time'], seed=7))
    exact = sampled = 0
    with hm.activate('k'):
        for b, batch in enumerate(DGDataLoader(dg, batch_size=bs, hook_manager=hm)):
            assert hasattr(batch, 'seed_node_nbr_mask')
            ev_hi = int(np.searchsorted(ts, ts[b * bs], side='left'))
            cnt = np.bincount(src[:ev_hi], minlength=n_nodes) + np.bincount(dst[:ev_hi], minlength=n_nodes)
            for h, k in enumerate(ks):
                seeds = batch.seed_nids[h].cpu().numpy()
                g_n, g_t, g_x = batch.nbr_nids[h], batch.nbr_edge_time[h], batch.nbr_edge_x[h]
                assert g_n.shape == g_t.shape == (len(seeds), k) and g_x.shape == (len(seeds), k, D)
                assert (g_n.dtype, g_t.dtype, g_x.dtype, batch.seed_times[h].dtype) == (torch.int32, torch.int64, torch.float32, torch.int64)
                if h:
                    assert torch.equal(batch.seed_nids[h], batch.nbr_nids[h - 1].view(-1))
                    assert torch.equal(batch.seed_times[h], batch.nbr_edge_time[h - 1].view(-1))
                o_n, o_t, o_x = uniform_ref.get_nbrs(src, dst, ts, edge_x, seeds, k, ev_hi, False)
                rows = np.asarray([s < 0 or cnt[s] <= k for s in seeds.tolist()])  # all neighbours, event order, left aligned
                assert np.array_equal(g_n.cpu().numpy()[rows], o_n[rows]) and np.array_equal(g_t.cpu().numpy()[rows], o_t[rows])
                assert g_x.cpu().numpy()[rows].tobytes() == o_x[rows].tobytes()
                assert (g_n.cpu().numpy()[~rows] >= 0).all()  # a sampled row has no pad
                exact, sampled = exact + int(rows.sum()), sampled + int((~rows).sum())
    assert exact > 0 and sampled > 0
