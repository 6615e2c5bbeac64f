"""GraphMixer on the device: TimeGapNeighborHook id for id against the reference fixtures and the restatement (loader settings, node
events, ties, self loops, repeated seeds, the last partial batch, splits, new epochs), MLPMixer and GraphMixerEncoder within the float
bar, bit-identity of the native call, the training path's gradients and checkpoint loading."""
import io
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_util import load
import graphmixer_restate as gr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4  # max |got - ref| / max(1, |ref|) against float64 (restatement) or the reference's float32 outputs


def _tgm():
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook, StatelessHook, TimeGapNeighborHook

    return SimpleNamespace(DGData=DGData, DGDataLoader=DGDataLoader, DGraph=DGraph, HookManager=HookManager, Neg=RandomNegativeEdgeSamplerHook,
                           Recency=RecencyNeighborHook, StatelessHook=StatelessHook, TimeGap=TimeGapNeighborHook)  # fmt: skip


def fixed_negatives_hook(neg: torch.Tensor):
    from tgm_amd.hooks import StatelessHook

    class FixedNegatives(StatelessHook):
        _cls_requires = {'edge_src', 'edge_dst', 'edge_time'}
        _cls_produces = {'neg', 'neg_time'}

        def __init__(self):
            super().__init__()
            self.__post_init__()

        def __call__(self, dg, batch):
            lo = dg._edge_range[0]
            n = batch.edge_src.numel()
            batch.neg = neg[lo : lo + n]
            batch.neg_time = batch.edge_time.clone()
            return batch

    return FixedNegatives()


def data_from_fixture(meta, a):
    """The reference's DGData input again (raw, unsorted ties and all), split like the fixture's stream."""
    t = _tgm()
    kw = {}
    if 'raw_node_t' in a:
        kw = dict(node_x_time=torch.from_numpy(a['raw_node_t']), node_x_nids=torch.from_numpy(a['raw_node_nids']), node_x=torch.from_numpy(a['raw_node_x']))
    data = t.DGData.from_raw(torch.from_numpy(a['raw_ts']), torch.from_numpy(a['raw_ei']), torch.from_numpy(a['raw_x']), **kw)
    data = data.split()[1] if meta['split'] else data
    st = t.DGraph(data)._storage
    assert np.array_equal(st._time_np, a['times']) and np.array_equal(st._edge_pos_np, a['edge_event'])  # the same timeline as the reference's
    return data


LOADERS = [dict(), dict(output_pool=0), dict(prefetch=1, output_pool=3, side_stream=True)]


@pytest.mark.parametrize('loader_kw', LOADERS, ids=['default', 'pool0', 'side_stream'])
@pytest.mark.parametrize('name', ['g15_graphmixer_hook_plain', 'g15_graphmixer_hook_nodes', 'g15_graphmixer_hook_split'])
def test_hook_matches_the_reference_fixture(name, loader_kw):
    t = _tgm()
    meta, a = load(name)
    dg = t.DGraph(data_from_fixture(meta, a), device=DEV)
    neg = torch.from_numpy(a['neg']).to(DEV)
    for gap in meta['gaps']:
        want = gr.unflatten(a[f'gap{gap}_vals'], a[f'gap{gap}_offs'])
        hm = t.HookManager(keys=['k'])
        hm.register('k', fixed_negatives_hook(neg))
        hm.register('k', t.TimeGap(gap))
        got = []
        with hm.activate('k'):
            for b in t.DGDataLoader(dg, batch_size=meta['batch_size'], hook_manager=hm, **loader_kw):
                assert b.time_gap_nbr.dtype == torch.int32 and b.time_gap_lo.numel() == 3 * b.edge_src.numel()
                got += gr.hook_lists(b.time_gap_nbr, b.time_gap_lo, b.time_gap_cnt)
        assert got == want, (name, gap, loader_kw)


def restated_lists(dg, start, bs, gap, batch):
    st = dg._storage
    times, epos = st._time_np, st._edge_pos_np
    src, dst = st._data.edge_index[:, 0].numpy(), st._data.edge_index[:, 1].numpy()
    lo = dg.slice_events(start, start + bs)._edge_range[0]
    if batch.edge_src.numel() == 0:
        return []
    seeds = torch.cat([batch.edge_src, batch.edge_dst, batch.neg]).cpu().numpy()
    return gr.time_gap_lists(times, epos, src, dst, start, start + bs, None, int(times[epos[lo]]), gap, seeds)


def wiki_graph(E=3050, D=8, node_events=False, seed=3):
    from tgm_amd.synth import make_stream

    t = _tgm()
    s = make_stream('wiki', seed=seed, num_edges=E, edge_dim=D, n_src=300, n_dst=100, t_hi=E // 2)  # 400 nodes, ~2 edges per timestamp
    src, dst = s.src.clone(), s.dst.clone()
    dst[::37] = src[::37]  # self loops
    kw = {}
    if node_events:
        g = torch.Generator().manual_seed(seed)
        M = E // 5
        kw = dict(node_x_time=torch.sort(torch.randint(0, E // 2, (M,), generator=g)).values, node_x_nids=torch.randint(0, 400, (M,), generator=g),
                  node_x=torch.rand((M, 2), generator=g))  # fmt: skip
    return t.DGData.from_raw(s.ts, torch.stack([src, dst], 1).int(), s.edge_x, **kw)


@pytest.mark.parametrize('gap', [0, 1, 2000, 10**9])
@pytest.mark.parametrize('node_events', [False, True])
def test_hook_matches_the_restatement_on_wiki_shaped_streams(gap, node_events):
    t = _tgm()
    data = wiki_graph(node_events=node_events)
    bs = 200
    for part in (data, data.split()[1]):  # the whole stream, then a split with its own timeline
        dg = t.DGraph(part, device=DEV)
        hm = t.HookManager(keys=['k'])
        hm.register('k', t.Neg(low=0, high=400))
        hm.register('k', t.Recency(400, [5], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
        hm.register('k', t.TimeGap(gap))
        lb = dg._event_range[0]
        for epoch in range(2):  # a reset_state / new-epoch run sees the same windows
            with hm.activate('k'):
                loader = t.DGDataLoader(dg, batch_size=bs, hook_manager=hm)
                starts = list(loader._starts)
                for s, b in zip(starts, loader):
                    assert gr.hook_lists(b.time_gap_nbr, b.time_gap_lo, b.time_gap_cnt) == restated_lists(dg, s, bs, gap, b), (gap, epoch, s)
                if part is data:
                    assert starts[-1] + bs > lb + dg.num_events  # the last batch is partial and keeps its nominal end
            hm.reset_state()


def mixer_from_fixture(name):
    from tgm_amd.nn import MLPMixer

    meta, a = load(name)
    m = MLPMixer(meta['K'], meta['C'], meta['token_expansion'], meta['channel_expansion'])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')})
    return m.to(DEV).eval(), a


@pytest.mark.parametrize('i', range(6))
def test_mlp_mixer_matches_the_reference_fixture(i):
    m, a = mixer_from_fixture(f'g15_graphmixer_mixer_{i}')
    with torch.no_grad():
        y = m(torch.from_numpy(a['x']).to(DEV))
    assert gr.rel_err(y, torch.from_numpy(a['y'])) < BAR


@pytest.mark.parametrize('K', [2, 5, 20, 30])
@pytest.mark.parametrize('C', [1, 16, 172, 200])
def test_mlp_mixer_odd_shapes(K, C):
    from tgm_amd.nn import MLPMixer

    torch.manual_seed(K * 1000 + C)
    for ft, fc in ((0.5, 4.0), (1.3, 0.7), (0.9, 2.3)):
        m = MLPMixer(K, C, ft, fc).to(DEV).eval()
        if int(fc * C) == 0:
            continue
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn_like(p))
            x = torch.randn(7, K, C, device=DEV) * 1.5
            y = m(x)
        sd = {k: v.cpu().double() for k, v in m.state_dict().items()}
        assert gr.rel_err(y, gr.mixer_forward(sd, '', x.cpu().double())) < BAR, (K, C, ft, fc)


def fixture_batch(a, bs):
    S = 3 * bs
    seeds = torch.from_numpy(a['seeds']).to(DEV)
    lists = gr.unflatten(a['tg_vals'], a['tg_offs'])
    offs = torch.from_numpy(a['tg_offs'])
    return SimpleNamespace(edge_src=seeds[:bs], edge_dst=seeds[bs : 2 * bs], neg=seeds[2 * bs :], nbr_edge_x=[torch.from_numpy(a['nbr_edge_x']).to(DEV)],
                           seed_times=[torch.from_numpy(a['seed_times']).to(DEV)], nbr_edge_time=[torch.from_numpy(a['nbr_edge_time']).to(DEV)],
                           nbr_nids=[torch.from_numpy(a['nbr_nids']).to(DEV)], time_gap_nbr=torch.from_numpy(a['tg_vals']).to(DEV),
                           time_gap_lo=offs[:S].int().to(DEV), time_gap_cnt=(offs[1:] - offs[:-1]).int().to(DEV)), lists  # fmt: skip


def test_encoder_matches_the_reference_fixture_and_loads_its_checkpoint():
    from tgm_amd.nn import GraphMixerEncoder

    meta, a = load('g15_graphmixer_encoder')
    buf = io.BytesIO()
    torch.save({k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')}, buf)
    buf.seek(0)
    enc = GraphMixerEncoder(**meta['dims'])
    enc.load_state_dict(torch.load(buf))
    enc = enc.to(DEV).eval()
    batch, _ = fixture_batch(a, meta['batch_size'])
    node_feat = torch.from_numpy(a['node_feat']).to(DEV)
    with torch.no_grad():
        z = enc(batch, node_feat)
    assert z.shape == (3 * meta['batch_size'], meta['dims']['embed_dim'])
    assert gr.rel_err(z, torch.from_numpy(a['z'])) < BAR


def sampled_batches(dims, E=2400, bs=200, gap=2000):
    t = _tgm()
    dg = t.DGraph(wiki_graph(E=E, D=dims['edge_dim']), device=DEV)
    hm = t.HookManager(keys=['k'])
    hm.register('k', t.Neg(low=0, high=400))
    hm.register('k', t.Recency(400, [dims['num_tokens']], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    hm.register('k', t.TimeGap(gap))
    with hm.activate('k'):
        return dg, list(t.DGDataLoader(dg, batch_size=bs, hook_manager=hm))


def restated_z(enc, batch, node_feat, dtype=torch.float64):
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    seeds = torch.cat([batch.edge_src, batch.edge_dst, batch.neg]).cpu()
    lists = gr.hook_lists(batch.time_gap_nbr, batch.time_gap_lo, batch.time_gap_cnt)
    return gr.encoder_forward(sd, enc.num_layers, batch.nbr_edge_x[0].cpu(), batch.seed_times[0].cpu(), batch.nbr_edge_time[0].cpu(),
                              batch.nbr_nids[0].cpu(), seeds, lists, node_feat.cpu(), dtype=dtype)  # fmt: skip


CFG2 = dict(time_dim=100, embed_dim=128, num_tokens=20, node_dim=100, edge_dim=172)


@pytest.mark.parametrize('dims', [CFG2, dict(time_dim=7, embed_dim=9, num_tokens=5, node_dim=3, edge_dim=13, num_layers=3, token_dim_expansion=1.3,
                                              channel_dim_expansion=2.1)], ids=['cfg2', 'odd'])  # fmt: skip
def test_encoder_end_to_end_on_sampler_output(dims, monkeypatch):
    from tgm_amd.nn import GraphMixerEncoder

    torch.manual_seed(0)
    dg, batches = sampled_batches(dims)
    enc = GraphMixerEncoder(**dims).to(DEV).eval()
    node_feat = torch.randn(400, dims['node_dim'], device=DEV)
    pads = 0
    for j in (0, 1, len(batches) - 1):  # the first batch (empty history: every slot padded), one more, the partial last one
        b = batches[j]
        pads += int((b.nbr_nids[0] == -1).sum())
        with torch.no_grad():
            z1 = enc(b, node_feat)
            z2 = enc(b, node_feat)
            monkeypatch.setenv('TGMX_GRAPHMIXER_PY', '1')
            z3 = enc(b, node_feat)
            monkeypatch.delenv('TGMX_GRAPHMIXER_PY')
        assert torch.equal(z1, z2) and torch.equal(z1, z3), j
        assert gr.rel_err(z1, restated_z(enc, b, node_feat)) < BAR, j
    assert pads > 0


def test_training_path_gradients():
    from tgm_amd.nn import GraphMixerEncoder

    dims = dict(time_dim=8, embed_dim=6, num_tokens=5, node_dim=4, edge_dim=12)
    torch.manual_seed(1)
    _, batches = sampled_batches(dims, E=1200, bs=100)
    b = batches[3]
    enc = GraphMixerEncoder(**dims, dropout=0.0).to(DEV).train()
    node_feat = torch.randn(400, dims['node_dim'], device=DEV)
    z = enc(b, node_feat)
    assert z.requires_grad
    (z * torch.linspace(-1, 1, z.numel(), device=DEV).view_as(z)).sum().backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.state_dict().items()}
    seeds = torch.cat([b.edge_src, b.edge_dst, b.neg]).cpu()
    lists = gr.hook_lists(b.time_gap_nbr, b.time_gap_lo, b.time_gap_cnt)
    zr = gr.encoder_forward(sd, enc.num_layers, b.nbr_edge_x[0].cpu(), b.seed_times[0].cpu(), b.nbr_edge_time[0].cpu(), b.nbr_nids[0].cpu(), seeds,
                            lists, node_feat.cpu())  # fmt: skip
    assert gr.rel_err(z, zr) < BAR
    (zr * torch.linspace(-1, 1, zr.numel(), dtype=torch.float64).view_as(zr)).sum().backward()
    for n, p in enc.named_parameters():
        if p.requires_grad:
            assert gr.rel_err(p.grad, sd[n].grad) < BAR, n
    with torch.no_grad():  # the same weights through the native inference call
        assert gr.rel_err(enc.eval()(b, node_feat), zr) < BAR


def _composed_spy(monkeypatch, module, took):
    torch_fwd = module._torch_forward
    monkeypatch.setattr(module, '_torch_forward', lambda *a, **k: took.append('composed') or torch_fwd(*a, **k))


@pytest.mark.parametrize('C,path', [(627, ['token']), (628, ['token', 'composed'])])
def test_mlp_mixer_at_the_edge_of_the_lds_envelope(C, path, monkeypatch):
    """tgmx_mixer_token keeps a seed's tile in 64 KiB of LDS: 4 * (K C + (K + Ht) * 128) bytes.  K = 20, Ht = 10: C = 627 (16 380 floats) is
    native, C = 628 answers TGMX_E_UNSUPPORTED and the eval-mode forward is the composed torch path -- it returns, within the bar."""
    from tgm_amd.nn import MLPMixer
    from tgm_amd.nn import mlp_mixer as mod

    torch.manual_seed(C)
    m = MLPMixer(20, C).to(DEV).eval()
    took = []
    token_block = mod.token_block
    monkeypatch.setattr(mod, 'token_block', lambda *a, **k: took.append('token') or token_block(*a, **k))
    _composed_spy(monkeypatch, m, took)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn_like(p))
        x = torch.randn(3, 20, C, device=DEV) * 1.5
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            y = m(x)
    assert took == path
    said = [w for w in caught if issubclass(w.category, RuntimeWarning) and 'not natively' in str(w.message)]
    assert len(said) == (1 if 'composed' in path else 0)  # the hand-over is not silent, and the native path says nothing
    assert y.shape == x.shape and not y.requires_grad
    sd = {k: v.cpu().double() for k, v in m.state_dict().items()}
    assert gr.rel_err(y, gr.mixer_forward(sd, '', x.cpu().double())) < BAR


@pytest.mark.parametrize('launches', [False, True], ids=['one_call', 'launches'])
def test_encoder_outside_the_lds_envelope_takes_the_composed_path(launches, monkeypatch):
    """num_tokens = 64 at edge_dim = 172: 23 296 floats of LDS per seed against 16 384.  The eval-mode encoder returns what the composed
    path computes (both the one-call forward and its launch-by-launch twin hand over), within the bar against the restatement."""
    from tgm_amd.nn import GraphMixerEncoder

    dims = dict(num_tokens=64, edge_dim=172, time_dim=8, node_dim=4, embed_dim=6)
    torch.manual_seed(2)
    _, batches = sampled_batches(dims, E=600, bs=50)
    b = batches[-2]
    assert int((b.nbr_nids[0] != -1).sum()) > 0
    enc = GraphMixerEncoder(**dims).to(DEV).eval()
    node_feat = torch.randn(400, dims['node_dim'], device=DEV)
    took = []
    _composed_spy(monkeypatch, enc, took)
    if launches:
        monkeypatch.setenv('TGMX_GRAPHMIXER_PY', '1')
    with torch.no_grad(), pytest.warns(RuntimeWarning, match='not natively'):  # the hand-over is not silent
        z = enc(b, node_feat)
    assert took == ['composed']
    assert z.shape == (3 * b.edge_src.numel(), dims['embed_dim']) and not z.requires_grad
    assert gr.rel_err(z, restated_z(enc, b, node_feat)) < BAR
