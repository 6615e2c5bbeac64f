"""TPNet on the device: the streaming update against the reference fixtures and the float64 restatement (parity, determinism, the
read-before-write ordering, reset / backup / reload), the pair features, the whole encoder (the ceiling, and the ratio to the reference's
own float32 distance), encode_pairs against forward on gathered tensors, an end-to-end stream through the sampler, the training path's
gradients, a reference-style training / evaluation step and the state_dict round trip.

Measured on an MI355X (max |got - ref| / max(1, |ref|) against float64; the reference's own float32 distance next to it): see DESIGN.md 3.6.
"""
import numpy as np
import pytest
import torch

from golden_util import load
import tpnet_restate as tr
from test_tpnet_cpu import (ENCODER_CASES, NOISE, PAIR_CASES, UPDATE_CASES, build_model, encoder_inputs, fixture_state_dict, restated, restated_stream,
                            rp_dict, rp_kwargs)  # fmt: skip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4  # the ceiling (tests/test_dygformer_gpu.py's)
RATIO = 2.0  # HIP's distance from float64 over the reference's own float32 distance from float64


def rp_from_update_fixture(meta, a):
    from tgm_amd.nn import RandomProjectionModule

    m = RandomProjectionModule(**rp_kwargs(meta['cfg']))
    with torch.no_grad():
        m.random_projections[0].copy_(torch.from_numpy(a['p0']))
    return m.to(DEV)


def run_stream(m, a, lo=0, hi=None):
    T = lambda v: torch.from_numpy(v).to(DEV)
    for b in range(lo, a['src'].shape[0] if hi is None else hi):
        m.update(T(a['src'][b]), T(a['dst'][b]), T(a['time'][b]))


@pytest.mark.parametrize('name', UPDATE_CASES)
def test_update_matches_the_reference_fixture_and_is_deterministic(name):
    meta, a = load(name)
    L = meta['cfg']['num_layer']
    m, m2 = rp_from_update_fixture(meta, a), rp_from_update_fixture(meta, a)
    run_stream(m, a)
    run_stream(m2, a)
    for i in range(L + 1):
        assert torch.equal(m.random_projections[i], m2.random_projections[i]), i  # two runs from one state: the same bits
    assert torch.equal(m.random_projections[0].cpu(), torch.from_numpy(a['p0']))  # level 0 is never written
    assert int(m.now_time) == meta['now'] and m.now_time.dtype == torch.int64 and m.now_time.dim() == 0
    r64, _ = restated_stream(meta, a)
    e64 = max(tr.rel_err(m.random_projections[i], r64[i]) for i in range(1, L + 1))
    efix = max(tr.rel_err(m.random_projections[i], torch.from_numpy(a[f'table_{i}'])) for i in range(1, L + 1))
    noise = NOISE['fixtures'][name]
    print(f'{name}: HIP vs float64 {e64:.3e}, reference float32 vs float64 {noise:.3e}, ratio {e64 / noise:.2f}; HIP vs the fixture {efix:.3e}')
    assert e64 < BAR and efix < BAR
    assert e64 <= RATIO * noise


def test_update_reads_the_previous_level_before_the_batch_touches_it():
    """Edge (0, 1) and edge (1, 2) in one batch: node 1 is a target (its level-1 row changes) and an endpoint (its level-1 row is the
    message for level 2).  Level 2 must see node 1's level-1 row as it was BEFORE this batch."""
    from tgm_amd.nn import RandomProjectionModule

    m = RandomProjectionModule(4, 2, 0.0, 0, use_matrix=True).to(DEV)
    T = lambda v, dt=torch.int64: torch.tensor(v, dtype=dt, device=DEV)
    m.update(T([0, 1]), T([1, 2]), T([5, 5]))
    P1, P2 = m.random_projections[1].cpu(), m.random_projections[2].cpu()
    want1 = torch.tensor([[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]], dtype=torch.float32)  # the adjacency matrix
    assert torch.equal(P1, want1)
    assert not P2.any()  # P[1] was zero before the batch: reading it after the batch's writes would put the adjacency's rows here
    m.update(T([2]), T([3]), T([6]))
    want2 = torch.zeros(4, 4)
    want2[2], want2[3] = want1[3], want1[2]  # two-step walks through the new edge, over the OLD one-step table
    assert torch.equal(m.random_projections[2].cpu(), want2)
    r, now = [torch.eye(4, dtype=torch.float64)] + [torch.zeros(4, 4, dtype=torch.float64)] * 2, 0
    for s, d, t in (([0, 1], [1, 2], [5, 5]), ([2], [3], [6])):
        r, now = tr.rp_update(r, now, s, d, t, 0.0)
    assert torch.equal(r[2].float(), want2)


def test_update_skips_edges_with_an_endpoint_outside_the_tables_and_accepts_int32():
    from tgm_amd.nn import RandomProjectionModule

    torch.manual_seed(0)
    m = RandomProjectionModule(6, 2, 1e-3, 0, use_matrix=False, enforce_dim=5).to(DEV)
    m2 = RandomProjectionModule(6, 2, 1e-3, 0, use_matrix=False, enforce_dim=5).to(DEV)
    m2.load_state_dict(m.state_dict())
    T = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    m.update(T([0, 9, 2, -1], torch.int32), T([1, 3, 7, 2], torch.int32), T([3, 4, 4, 9], torch.int64))
    m2.update(T([0], torch.int64), T([1], torch.int64), T([9], torch.int64))
    m2w = np.exp(-1e-3 * 6)  # the one valid edge sits at t = 3, the batch ends at t = 9
    assert int(m.now_time) == 9
    assert tr.rel_err(m.random_projections[1], m2.random_projections[1] * m2w) < 1e-6


def test_reset_backup_reload_round_trip_bit_for_bit():
    meta, a = load('g17_tpnet_update_rand_l2')
    m = rp_from_update_fixture(meta, a)
    run_stream(m, a, 0, 10)
    saved = m.backup_random_projections()
    keep = [p.clone() for p in m.random_projections]
    run_stream(m, a, 10, 20)
    after20 = [p.clone() for p in m.random_projections]
    m.reload_random_projections(saved)
    assert int(m.now_time) == int(saved[0]) and all(torch.equal(p, q) for p, q in zip(m.random_projections, keep))
    run_stream(m, a, 10, 20)
    assert all(torch.equal(p, q) for p, q in zip(m.random_projections, after20))  # the same ten batches from the reloaded state: the same bits
    m.reset_random_projections(reset_zero=False)
    assert int(m.now_time) == meta['cfg']['beginning_time'] and not m.random_projections[1].any() and not m.random_projections[2].any()
    assert torch.equal(m.random_projections[0], keep[0])
    run_stream(m, a, 0, 10)
    assert all(torch.equal(p, q) for p, q in zip(m.random_projections, keep))
    sd = {k: v.clone() for k, v in m.state_dict().items()}  # the materialised values
    assert torch.equal(sd['random_projections.2'], keep[2]) and torch.equal(m.get_random_projections(torch.tensor([3, -1], device=DEV))[:, 2], keep[2][[3, -1]])


def pair_module(meta, a):
    from tgm_amd.nn import RandomProjectionModule

    m = RandomProjectionModule(**rp_kwargs(meta['cfg']))
    m.load_state_dict(fixture_state_dict(meta, a), strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize('name', PAIR_CASES)
def test_pair_features_match_the_reference_fixture(name):
    meta, a = load(name)
    cfg = meta['cfg']
    m = pair_module(meta, a)
    sd = fixture_state_dict(meta, a)
    ia, ib = torch.from_numpy(a['a']).to(DEV), torch.from_numpy(a['b']).to(DEV)
    with torch.no_grad():
        out = m(ia, ib)
        raw = m.random_feature(ia.long(), ib.long())
        out2 = m(ia, ib)
    assert torch.equal(out, out2)
    tabs = [sd[f'random_projections.{i}'] for i in range(cfg['num_layer'] + 1)]
    f64 = tr.rp_features(tabs, a['a'], a['b'], cfg.get('concat', True), cfg.get('scale', True))
    f32 = tr.rp_features(tabs, a['a'], a['b'], cfg.get('concat', True), cfg.get('scale', True), dtype=torch.float32)
    eraw, nraw = tr.rel_err(raw, f64), tr.rel_err(f32, f64)
    e64 = tr.rel_err(out, tr.rp_forward(sd, '', cfg['num_layer'], a['a'], a['b'], cfg.get('concat', True), cfg.get('scale', True)))
    efix = tr.rel_err(out, torch.from_numpy(a['out']))
    noise = NOISE['fixtures'][name]
    print(f'{name}: kernel vs float64 {eraw:.3e} (float32 restatement {nraw:.3e}); after the MLP HIP vs float64 {e64:.3e}, reference float32 vs float64 '
          f'{noise:.3e}, ratio {e64 / noise:.2f}; HIP vs the fixture {efix:.3e}')
    assert e64 < BAR and efix < BAR
    assert e64 <= RATIO * noise
    assert eraw <= RATIO * max(nraw, 2.0**-23)  # the kernel alone, against the same arithmetic in float32 torch
    g = m(ia, ib)  # gradients enabled: the composed path
    assert g.requires_grad and tr.rel_err(g, out) < 1e-5


def test_pair_features_beyond_four_tables_take_the_composed_path():
    from tgm_amd.nn import RandomProjectionModule

    torch.manual_seed(1)
    m = RandomProjectionModule(12, 4, 1e-3, 0, use_matrix=False, enforce_dim=6, concat_src_dst=False).to(DEV).eval()
    T = lambda v: torch.tensor(v, device=DEV)
    for b in range(4):
        m.update(T([b, b + 1, 2]), T([b + 2, 0, 5]), T([10 * b, 10 * b + 1, 10 * b + 5]))
    assert m.random_projections[4].any()  # the update is native for every level
    with torch.no_grad():
        out = m(T([0, 3, -1]), T([2, 2, 4]))
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    assert tr.rel_err(out, tr.rp_forward(sd, '', 4, [0, 3, -1], [2, 2, 4], False, True)) < 1e-5


def run_forward(m, i):
    dev = lambda t: t.to(DEV)
    return m(dev(i['node_x']), torch.stack([dev(i['src']), dev(i['dst'])]), dev(i['edge_time']), dev(i['nbr_nids']), dev(i['nbr_time']), dev(i['nbr_edge_x']))


def model_from_fixture(meta, a):
    sd = fixture_state_dict(meta, a)
    m = build_model(meta)
    m.load_state_dict(sd, strict=True)  # a reference state_dict (its now_time has shape [1] after an update) loads strictly
    return m.to(DEV).eval(), sd


@pytest.mark.parametrize('name', ENCODER_CASES)
def test_encoder_matches_the_reference_fixture(name, monkeypatch):
    meta, a = load(name)
    m, sd = model_from_fixture(meta, a)
    i = encoder_inputs(a)
    took = []
    orig = m._forward_native
    monkeypatch.setattr(m, '_forward_native', lambda *x: took.append(1) or orig(*x))
    with torch.no_grad():
        zs, zd = run_forward(m, i)
        zs2, zd2 = (t.clone() for t in run_forward(m, i))
    assert took == [1, 1]  # the native call, twice, and no hand-over to the composed path
    assert torch.equal(zs, zs2) and torch.equal(zd, zd2)
    rs, rd = restated(meta, a, sd)
    e64 = max(tr.rel_err(zs, rs), tr.rel_err(zd, rd))
    efix = max(tr.rel_err(zs, torch.from_numpy(a['z_src'])), tr.rel_err(zd, torch.from_numpy(a['z_dst'])))
    noise = NOISE['fixtures'][name]
    print(f'{name}: HIP vs float64 {e64:.3e}, reference float32 vs float64 {noise:.3e}, ratio {e64 / noise:.2f}; HIP vs the fixture {efix:.3e}')
    assert e64 < BAR and efix < BAR
    assert e64 <= RATIO * noise
    back = {k: v.cpu() for k, v in m.state_dict().items()}  # ... and back: keys, dtypes and values as loaded
    assert list(back) == meta['state_dict_keys'] and all(back[k].dtype == sd[k].dtype and torch.equal(back[k].reshape(-1), sd[k].reshape(-1)) for k in sd)


def test_the_two_reference_quirks():
    """Pad tokens are NOT zeroed after the projection, and pad slots carry the pair features of node num_nodes - 1."""
    meta, a = load('g17_tpnet_enc_padheavy')
    m, sd = model_from_fixture(meta, a)
    i = encoder_inputs(a)
    assert (i['nbr_nids'][0] == -1).all()
    with torch.no_grad():
        zs, zd = run_forward(m, i)
        # an all-pad sequence is not the mixer's answer to zero tokens: its tokens went through the projection's biases, the edge
        # features the sampler left and the pair features of the last node
        zero_tokens = torch.zeros(1, meta['dims']['num_neighbors'], meta['dims']['output_dim'], device=DEV)
        for mx in m.mlp_mixers:
            zero_tokens = mx(zero_tokens)
        assert tr.rel_err(zs[0], zero_tokens.mean(dim=1)[0]) > 1e-3
        # the same input with the pads spelled as the last node's id gives the same pair-feature columns: compare through a model whose
        # node and time columns do not see the difference (node_x's last row zeroed is not enough: time is zeroed only for pads), so check
        # the pair features directly
        rp = m.random_projections
        n_last = meta['cfg']['num_nodes'] - 1
        pads = torch.full((5,), -1, device=DEV)
        assert torch.equal(rp(pads, torch.arange(5, device=DEV)), rp(torch.full((5,), n_last, device=DEV), torch.arange(5, device=DEV)))
        # and changing the last node's rows changes the all-pad sequence's embedding
        for p in rp.random_projections:
            p[-1] = p[0]
        zs3, _ = run_forward(m, i)
    assert tr.rel_err(zs3[0], zs[0]) > 1e-5
    rs, rd = restated(meta, a, sd)
    assert max(tr.rel_err(zs, rs), tr.rel_err(zd, rd)) < BAR


def wiki_batches(E=2400, bs=200, k=32, D=172, N=400):
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook
    from tgm_amd.synth import make_stream

    s = make_stream('wiki', seed=5, num_edges=E, edge_dim=D, n_src=300, n_dst=100, t_hi=E * 20)
    dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1).int(), s.edge_x), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
    hm.register('k', RecencyNeighborHook(N, [k], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    with hm.activate('k'):
        return list(DGDataLoader(dg, batch_size=bs, hook_manager=hm))


def pair_rows(b, negatives: bool):
    """The example's pair assembly as row indices into hop 0 (seeds edge_src | edge_dst | neg)."""
    n = b.edge_src.numel()
    ar = torch.arange(n, device=DEV, dtype=torch.int32)
    return ar, (ar + 2 * n if negatives else ar + n)


def gathered(b, src_rows, dst_rows):
    rows = torch.cat([src_rows, dst_rows]).long()
    return b.nbr_nids[0][rows], b.nbr_edge_time[0][rows], b.nbr_edge_x[0][rows]


def cpu_state(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def cpu_restated(m, sd, node_x, src, dst, t, nids, nt, nx, dtype=torch.float64):
    c = lambda v: v.detach().cpu()
    rp = m.random_projections
    rpd = None if rp is None else dict(num_layer=rp.num_layer, concat=rp.concat_src_dst, scale=rp.scale)
    return tr.tpnet_forward(sd, m.num_layers, rpd, c(node_x), c(src), c(dst), c(t), c(nids), c(nt), c(nx), dtype=dtype)


def example_model(N, concat=True, **dims):
    from tgm_amd.nn import RandomProjectionModule, TPNet

    rp = RandomProjectionModule(N, 2, 1e-6, 0, use_matrix=False, num_edges=110_000, dim_factor=10, concat_src_dst=concat)
    d = dict(node_feat_dim=128, edge_x_dim=172, time_feat_dim=100, output_dim=172, num_neighbors=32, num_layers=2, dropout=0.1)
    d.update(dims)
    return TPNet(**d, random_projections=rp, device=DEV).to(DEV).eval()


@pytest.mark.parametrize('concat', [True, False], ids=['concat', 'cross'])
def test_end_to_end_stream_through_the_sampler(concat):
    """Sampler -> native forward (positive and negative call) -> update, batch after batch; the same loop from torch ops in float64 on the
    CPU, fed the same sampler output, stays within the ratio rule at the last batch (the float32 restatement stands in for the reference).

    Batch 1 (one batch of history: a third of the sequences are all pads) is held to the same rule.  The K tokens of an all-pad sequence are
    identical, so every column the token LayerNorm sees is constant: float64 normalises it to exactly 0, and an error d in the column's
    float32 mean would come out as d / sqrt(eps) = 316 d.  tgmx_tpnet_token_mix corrects the mean once (mean += sum(x - mean) / K), which
    returns the mean of K equal values bit for bit; see DESIGN.md 3.6 for the figures with and without the correction."""
    torch.manual_seed(0)
    batches = wiki_batches()
    m = example_model(400, concat)
    assert m.random_projections.dim == 120
    node_x = torch.randn(400, 128, device=DEV)
    sd = cpu_state(m)
    L = m.random_projections.num_layer
    key = lambda i: f'random_projections.random_projections.{i}'
    t64, t32, now = [sd[key(i)].double() for i in range(L + 1)], [sd[key(i)].clone() for i in range(L + 1)], 0
    for j, b in enumerate(batches):
        last = j == len(batches) - 1
        for negatives in (False, True):
            sr, dr_ = pair_rows(b, negatives)
            src, dst = b.edge_src, (b.neg if negatives else b.edge_dst)
            with torch.no_grad():
                es, ed = m.encode_pairs(node_x, src, dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr_)
            if last or j == 1:
                nids, nt, nx = gathered(b, sr, dr_)
                with torch.no_grad():
                    zs, zd = m(node_x, torch.stack([src, dst]), b.edge_time, nids, nt, nx)
                assert torch.equal(zs, es) and torch.equal(zd, ed), j  # encode_pairs = forward on gathered tensors
                sd64 = dict(sd, **{key(i): t64[i] for i in range(L + 1)})
                sd32 = dict(sd, **{key(i): t32[i] for i in range(L + 1)})
                r64 = cpu_restated(m, sd64, node_x, src, dst, b.edge_time, nids, nt, nx)
                r32 = cpu_restated(m, sd32, node_x, src, dst, b.edge_time, nids, nt, nx, dtype=torch.float32)
                e64 = max(tr.rel_err(es, r64[0]), tr.rel_err(ed, r64[1]))
                n32 = max(tr.rel_err(r32[0], r64[0]), tr.rel_err(r32[1], r64[1]))
                print(f'batch {j} negatives={negatives}: HIP vs float64 {e64:.3e}, float32 restatement vs float64 {n32:.3e}, ratio {e64 / n32:.2f}')
                assert e64 < BAR and e64 <= RATIO * n32, j
        m.random_projections.update(b.edge_src, b.edge_dst, b.edge_time)
        c = lambda v: v.cpu()
        t64, nxt = tr.rp_update(t64, now, c(b.edge_src), c(b.edge_dst), c(b.edge_time), 1e-6)
        t32, _ = tr.rp_update(t32, now, c(b.edge_src), c(b.edge_dst), c(b.edge_time), 1e-6, dtype=torch.float32)
        now = nxt
    e_tab = max(tr.rel_err(m.random_projections.random_projections[i], t64[i]) for i in range(1, L + 1))
    n_tab = max(tr.rel_err(t32[i], t64[i]) for i in range(1, L + 1))
    print(f'tables after {len(batches)} batches: HIP vs float64 {e_tab:.3e}, float32 restatement vs float64 {n_tab:.3e}')
    assert e_tab < BAR and e_tab <= RATIO * n_tab and int(m.random_projections.now_time) == now


def test_encode_pairs_one_vs_many_equals_forward_on_gathered_tensors():
    from tgm_amd.nn import RandomProjectionModule, TPNet

    torch.manual_seed(1)
    batches = wiki_batches(E=1200, bs=100, k=6, D=12)
    b = batches[6]
    rp = RandomProjectionModule(400, 2, 1e-5, 0, use_matrix=False, enforce_dim=9)
    m = TPNet(9, 12, 10, 14, 6, num_layers=2, random_projections=rp, device=DEV).to(DEV).eval()
    for pb in batches[:6]:
        rp.update(pb.edge_src, pb.edge_dst, pb.edge_time)
    node_x = torch.randn(400, 9, device=DEV)
    n = b.edge_src.numel()
    # the example's evaluation step: ONE positive edge against every negative of its list (neg.shape[0] != edge_src.shape[0])
    for pos in (0, 17):
        M = 40
        src_rows = torch.full((M,), pos, dtype=torch.int32, device=DEV)  # edge_src repeat_interleave'd
        dst_rows = torch.arange(2 * n, 2 * n + M, dtype=torch.int32, device=DEV)  # rows of the negatives
        seeds = torch.cat([b.edge_src, b.edge_dst, b.neg])
        src, dst, t = seeds[src_rows.long()], seeds[dst_rows.long()], b.edge_time[pos].repeat(M)
        nids, nt, nx = gathered(b, src_rows, dst_rows)
        with torch.no_grad():
            zs, zd = m(node_x, torch.stack([src, dst]), t, nids, nt, nx)
            es, ed = m.encode_pairs(node_x, src, dst, t, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], src_rows, dst_rows)
        assert torch.equal(zs, es) and torch.equal(zd, ed)
        r = cpu_restated(m, cpu_state(m), node_x, src, dst, t, nids, nt, nx)
        assert max(tr.rel_err(zs, r[0]), tr.rel_err(zd, r[1])) < BAR


def test_training_path_gradients():
    from tgm_amd.nn import RandomProjectionModule, TPNet

    torch.manual_seed(4)
    batches = wiki_batches(E=1200, bs=100, k=7, D=12)
    b = batches[3]
    rp = RandomProjectionModule(400, 2, 1e-5, 0, use_matrix=False, enforce_dim=8)
    m = TPNet(4, 12, 8, 10, 7, num_layers=2, dropout=0.0, random_projections=rp, device=DEV).to(DEV).train()
    for pb in batches[:3]:
        rp.update(pb.edge_src, pb.edge_dst, pb.edge_time)
    node_x = torch.randn(400, 4, device=DEV)
    sr, dr_ = pair_rows(b, True)
    nids, nt, nx = gathered(b, sr, dr_)
    zs, zd = m(node_x, torch.stack([b.edge_src, b.neg]), b.edge_time, nids, nt, nx)
    assert zs.requires_grad
    z = torch.cat([zs, zd])
    (z * torch.linspace(-1, 1, z.numel(), device=DEV).view_as(z)).sum().backward()
    sd = {k: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}
    rs, rd = cpu_restated(m, sd, node_x, b.edge_src, b.neg, b.edge_time, nids, nt, nx)
    zr = torch.cat([rs, rd])
    assert tr.rel_err(z, zr) < BAR
    (zr * torch.linspace(-1, 1, zr.numel(), dtype=torch.float64).view_as(zr)).sum().backward()
    checked = 0
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert tr.rel_err(p.grad, sd[n].grad) < BAR, n
            checked += 1
    assert checked >= 2 + 4 + 4 + 2 * 12  # time encoder, pair-feature MLP, projection, two mixers
    with torch.no_grad():  # the same weights through the native inference call
        es, ed = m.eval()(node_x, torch.stack([b.edge_src, b.neg]), b.edge_time, nids, nt, nx)
    assert tr.rel_err(torch.cat([es, ed]), zr) < BAR


def test_reference_style_training_and_evaluation_step(monkeypatch):
    """``from tgm.nn import TPNet`` / ``from tgm.nn.encoder.tpnet import RandomProjectionModule`` with tgm -> tgm_amd: construct, load a
    reference state_dict, forward, BCE, backward, Adam, update, then an eval-mode step."""
    import sys

    import tgm_amd

    monkeypatch.setitem(sys.modules, 'tgm', tgm_amd)
    monkeypatch.setitem(sys.modules, 'tgm.nn', tgm_amd.nn)
    monkeypatch.setitem(sys.modules, 'tgm.nn.encoder', tgm_amd.nn.encoder)
    monkeypatch.setitem(sys.modules, 'tgm.nn.encoder.tpnet', tgm_amd.nn.tpnet)
    from tgm.nn import TPNet
    from tgm.nn.encoder.tpnet import RandomProjectionModule

    meta, a = load('g17_tpnet_enc_small')
    rp = RandomProjectionModule(**rp_kwargs(meta['cfg']), device=DEV)
    m = TPNet(**meta['dims'], random_projections=rp, device=DEV)
    m.load_state_dict(fixture_state_dict(meta, a), strict=True)
    m = m.to(DEV)
    rp_module = rp.to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    i = encoder_inputs(a)
    m.train()
    zs, zd = run_forward(m, i)
    logit = (zs * zd).sum(dim=1)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.ones_like(logit))
    loss.backward()
    opt.step()
    before = rp_module.random_projections[1].clone()
    rp_module.update(i['src'].to(DEV), i['dst'].to(DEV), i['edge_time'].sort().values.to(DEV) + 10**6)
    assert not torch.equal(before, rp_module.random_projections[1])
    m.eval()
    with torch.no_grad():
        es, ed = run_forward(m, i)
    sd = cpu_state(m)
    rs, rd = restated(meta, a, sd)
    assert es.shape == zs.shape and max(tr.rel_err(es, rs), tr.rel_err(ed, rd)) < BAR  # the native call sees the updated weights and tables
    assert not torch.equal(es, zs.detach())
