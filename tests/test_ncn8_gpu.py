"""NCNPredictor at k = 8 on the device: the native two-hop stage against the reference fixtures and the float64 restatement, the native path
and its bits (two runs, prepared adjacency, int32 / strided / reordered edge lists, int32 targets), LDS against workspace storage, 'all'
against 'last', the edge cases, the composed path's gradients, an end-to-end stream at the example's shape and the reference's own three
tests.  Every test here needs the k = 8 stage: before it existed ``forward`` raised ``NotImplementedError``.

Every parity test prints HIP's distance from float64 (max |got - ref| / max(1, |ref|)) next to the reference's own float32 distance and their
ratio; the measured figures are in DESIGN.md 3.7.
"""
import pytest
import torch

from golden_util import load
import ncn8_restate as n8
import ncn_restate as nr
from test_ncn8_cpu import CASES8, NOISE8, recorded_rows
from test_ncn_cpu import CN_BAR, LOGIT_BAR, fixture_inputs
from test_ncn_gpu import DEV, check_against_float64, dev, model_from_fixture, reordered, run

pytestmark = pytest.mark.gpu


def same(got, base):
    return torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


@pytest.mark.parametrize('name', CASES8)
def test_native_forward_matches_the_reference_fixture(name, monkeypatch):
    meta, a = load(name)
    m, sd = model_from_fixture(meta, a)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    took = []
    orig = m._native_xs
    monkeypatch.setattr(m, '_native_xs', lambda *p, **q: took.append(1) or orig(*p, **q))
    cn, out = run(m, dev(x), dev(ei), dev(tar), dev(lu), dev(et))
    cn2, out2 = run(m, dev(x), dev(ei), dev(tar), dev(lu), dev(et))
    assert took == [1] * 4  # the native path, no hand-over to torch ops
    assert torch.equal(cn, cn2) and torch.equal(out, out2)  # two runs, the same bits
    assert cn.shape == (tar.shape[1], 7 * meta['C'])
    check_against_float64(name, 'cn_emb', cn, n8.cn_emb(x, ei, tar, lu, et), NOISE8[name]['cn_emb'], CN_BAR)
    check_against_float64(name, 'logits', out, n8.forward(sd, x, ei, tar, lu, et), NOISE8[name]['logits'], LOGIT_BAR)
    assert nr.rel_err(recorded_rows(meta, cn), torch.from_numpy(a['cn_emb'])) < CN_BAR and nr.rel_err(out, torch.from_numpy(a['logits'])) < LOGIT_BAR


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_hub'])
def test_edge_list_forms_and_the_prepared_adjacency_give_the_same_bits(name):
    from tgm_amd.nn.ncn import adjacency

    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    E = ei.shape[1]
    base = run(m, x, ei.contiguous(), tar, lu, et)
    assert base[0].any()
    buf = torch.full((2, E + 37), 10**6, dtype=torch.long, device=DEV)  # what lies behind the view is never a valid id
    buf[:, :E] = ei
    view = buf[:, :E]
    assert not view.is_contiguous()
    for variant in (view, ei.int(), buf.int()[:, :E], reordered(ei), adjacency(meta['N'], ei), adjacency(meta['N'], reordered(ei).int())):
        assert same(run(m, x, variant, tar, lu, et), base)
    assert same(run(m, x, ei, tar.int(), lu, et), base)
    adj = adjacency(meta['N'], ei)
    for _ in range(3):  # one build, many calls
        assert same(run(m, x, adj, tar, lu, et), base)


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_hub', 'g34_ncn8_width_c300', 'g34_ncn8_selfloop_plain'])
@pytest.mark.parametrize('dup', ['last', 'all'])
def test_lds_and_workspace_storage_give_the_same_bits(name, dup):
    """The same kernel over LDS rows and over workspace rows (forced on shapes that fit LDS; g34_ncn8_wide_n7681 in the fixture test takes the
    workspace form by its size)."""
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a, duplicate_targets=dup)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    W = 8 * meta['C']
    with torch.no_grad():
        lds = m._native_xs(m._inputs(x, ei, tar, lu, et), mlp=False)[0][:, :W].clone()
        ws = m._native_xs(m._inputs(x, ei, tar, lu, et), mlp=False, force_workspace=True)[0][:, :W].clone()
        ws2 = m._native_xs(m._inputs(x, ei, tar, lu, et), mlp=False, force_workspace=True)[0][:, :W].clone()
    assert lds[:, meta['C'] :].any() and torch.equal(lds, ws) and torch.equal(ws, ws2)
    ref = n8.cn_emb(x.cpu(), ei.cpu(), tar.cpu(), None if lu is None else lu.cpu(), None if et is None else et.cpu(), duplicate_targets=dup)
    assert nr.rel_err(ws[:, meta['C'] :], ref) < CN_BAR


def test_workspace_regions_are_reused_across_pairs():
    """More pairs than resident workgroups (256): a region serves several pairs, each finding it as the one before left it -- zeroed."""
    meta, a = load('g34_ncn8_triangle_decay')
    m, _ = model_from_fixture(meta, a, duplicate_targets='all')
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    reps = 60  # 9 pairs x 60 = 540 > 2 x 256
    tar_many, et_many = tar.repeat(1, reps), et.repeat(reps)
    W = 8 * meta['C']
    with torch.no_grad():
        one = m._native_xs(m._inputs(x, ei, tar, lu, et), mlp=False)[0][:, :W].clone()
        many = m._native_xs(m._inputs(x, ei, tar_many, lu, et_many), mlp=False, force_workspace=True)[0][:, :W].clone()
    assert one[:, meta['C'] :].any() and torch.equal(many, one.repeat(reps, 1))


def test_all_equals_last_on_single_pairs():
    meta, a = load('g34_ncn8_onevsmany_decay')
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    m_all, sd = model_from_fixture(meta, a, duplicate_targets='all')
    m_last, _ = model_from_fixture(meta, a)
    cn_all, out_all = run(m_all, x, ei, tar, lu, et)
    cn_last, _ = run(m_last, x, ei, tar, lu, et)
    assert not cn_last[:-1].any() and cn_all.any(dim=1).sum() > 3  # one source repeated: 'last' keeps the last candidate only
    for r in range(tar.shape[1]):
        cn1, out1 = run(m_last, x, ei, tar[:, r : r + 1], lu, et[r : r + 1])
        assert torch.equal(cn1[0], cn_all[r]) and torch.equal(out1, out_all[r : r + 1]), r
    ref = n8.forward(sd, x.cpu(), ei.cpu(), tar.cpu(), lu.cpu(), et.cpu(), duplicate_targets='all')
    assert nr.rel_err(out_all, ref) < LOGIT_BAR


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_plain', 'g34_ncn8_rand_decay'])
def test_targets_outside_the_node_table_give_zero_rows_on_both_paths(name):
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    bad = tar.clone()
    bad[0, 2], bad[1, 5] = meta['N'], -1
    W = 8 * meta['C']
    with torch.no_grad():
        xs = m._native_xs(m._inputs(x, ei, bad, lu, et), mlp=False)[0][:, :W].clone()
        out = m(x, ei, bad, lu, et)
    assert not xs[2].any() and not xs[5].any() and xs[-1, meta['C'] :].any()
    # the other rows are what the call without the two pairs gives: an id outside the table marks no last occurrence
    rest = [r for r in range(tar.shape[1]) if r not in (2, 5)]
    with torch.no_grad():
        xs_rest = m._native_xs(m._inputs(x, ei, bad[:, rest], lu, et[rest] if et is not None else None), mlp=False)[0][:, :W]
    assert torch.equal(xs[rest], xs_rest)
    m.train()  # the composed path: the same rows, no device-side assert
    composed = m._torch_xs(m._inputs(x, ei, bad, lu, et))
    assert not composed[2].any() and not composed[5].any() and nr.rel_err(composed, xs) < CN_BAR
    assert nr.rel_err(m(x, ei, bad, lu, et), out) < LOGIT_BAR


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_hub'])
def test_edges_with_an_endpoint_outside_the_node_table_are_left_out(name):
    from tgm_amd.nn.ncn import adjacency

    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    N = meta['N']
    extra = torch.tensor([[N, 0, -1, 2**31 - 1], [1, N + 5, 3, 0]], device=DEV)
    more = torch.cat([extra[:, :2], ei, extra[:, 2:]], dim=1)
    base = run(m, x, ei, tar, lu, et)
    assert same(run(m, x, more, tar, lu, et), base) and same(run(m, x, adjacency(N, more), tar, lu, et), base)
    m.train()
    want = m._torch_xs(m._inputs(x, ei, tar, lu, et))
    assert nr.rel_err(m._torch_xs(m._inputs(x, more, tar, lu, et)), want) == 0.0
    # the composed path through the prepared adjacency walks all 2 E slots, the eight dropped ones behind the last row included
    assert nr.rel_err(m._torch_xs(m._inputs(x, adjacency(N, more), tar, lu, et)), want) == 0.0


@pytest.mark.parametrize('N', [1, 5])
def test_degenerate_shapes(N):
    from tgm_amd.nn import NCNPredictor

    torch.manual_seed(N + 8)
    m = NCNPredictor(1, 3, 1, k=8).to(DEV).eval()
    x = torch.randn(N, 1, device=DEV)
    ei = torch.zeros((2, 0), dtype=torch.long, device=DEV)
    tar = torch.tensor([[0], [N - 1]], device=DEV)
    cn, out = run(m, x, ei, tar, None, None)
    assert cn.shape == (1, 7) and not cn.any()  # N = 1 and E = 0: a zero cn_emb
    sd = {n: v.cpu() for n, v in m.state_dict().items()}
    assert nr.rel_err(out, n8.forward(sd, x.cpu(), ei.cpu(), tar.cpu())) < 1e-6
    with torch.no_grad():
        empty = torch.zeros((2, 0), dtype=torch.long, device=DEV)
        assert m(x, ei, empty).shape == (0,) and m.get_cn_emb(x, ei, empty, (None, None)).shape == (0, 7)  # B = 0
    loop = torch.zeros((2, 3), dtype=torch.long, device=DEV)  # N = 1 with three self-loops: A = [[6]]
    if N == 1:
        cn, out = run(m, x, loop, tar, None, None)
        assert nr.rel_err(cn, n8.cn_emb(x.cpu(), loop.cpu(), tar.cpu())) < CN_BAR and cn.any()


def test_time_decay_corners():
    meta, a = load('g34_ncn8_decay_edges')
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    W = nr.decay_weights(lu, et)
    assert (W == 0).any() and (W == 1).any() and (W > 1).any() and torch.isfinite(W).all()  # underflow to 0, gaps of 0, a negative finite gap
    m, _ = model_from_fixture(meta, a)
    cn, _ = run(m, dev(x), dev(ei), dev(tar), dev(lu), dev(et))
    assert nr.rel_err(cn, n8.cn_emb(x, ei, tar, lu, et)) < CN_BAR
    assert nr.rel_err(cn, n8.cn_emb(x, ei, tar)) > 1e-3  # ... and the weights do matter here
    C = meta['C']
    plain, _ = run(model_from_fixture(dict(meta, decay=False), a)[0], dev(x), dev(ei), dev(tar), None, None)
    assert torch.equal(cn[:, 6 * C :], plain[:, 6 * C :]) and plain[:, 6 * C :].any()  # special_2_2 carries no decay


def test_an_infinite_weight_leaves_zero_counts_alone():
    """The one behaviour of the reference that is not reproduced: its dense c o W turns 0 * inf into NaN over the whole row."""
    meta, a = load('g34_ncn8_triangle_decay')
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    base = run(m, x, ei, tar, lu, et)
    # one more node, in no edge and no pair, last updated far in the future: W[:, N] = exp(1e4) = inf in float32
    x1 = torch.cat([x, torch.ones((1, meta['C']), device=DEV)])
    lu1 = torch.cat([lu, et.max().reshape(1) + 10**8])
    assert torch.isinf(nr.decay_weights(lu1.cpu(), et.cpu(), torch.float32)[:, -1]).all()
    got = run(m, x1, ei, tar, lu1, et)
    assert same(got, base) and torch.isfinite(got[0]).all()
    m.train()
    composed = m._torch_xs(m._inputs(x1, ei, tar, lu1, et))[:, meta['C'] :]
    assert torch.isfinite(composed).all() and nr.rel_err(composed, got[0]) < CN_BAR  # the composed path agrees


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_selfloop_plain', 'g34_ncn8_hub'])
def test_composed_path_gradients(name, monkeypatch):
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    m.train()
    monkeypatch.setattr(m, '_native_xs', lambda *p, **q: pytest.fail('the native stage has no backward at k = 8'))
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    xd = dev(x).requires_grad_(True)
    out = m(xd, dev(ei), dev(tar), dev(lu), dev(et))
    assert out.requires_grad
    wts = torch.linspace(-1, 1, out.numel(), dtype=torch.float64)
    (out * wts.to(DEV).float()).sum().backward()
    sd = {n: v.detach().cpu().double().requires_grad_(True) for n, v in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    ref = n8.forward(sd, x64, ei, tar, lu, et)
    assert nr.rel_err(out, ref) < LOGIT_BAR
    (ref * wts).sum().backward()
    bar = lambda g: 1e-4 * float(g.abs().max())  # the project's gradient bar: 1e-4 of each gradient's max
    assert float((xd.grad.cpu().double() - x64.grad).abs().max()) <= bar(x64.grad)
    for n, p in m.named_parameters():
        if n.startswith('xslin'):
            assert p.grad is None and sd[n].grad is None  # unused in forward
        else:
            assert float((p.grad.cpu().double() - sd[n].grad).abs().max()) <= bar(sd[n].grad), n
    monkeypatch.undo()
    with torch.no_grad():  # the same weights through the native call
        assert nr.rel_err(m.eval()(dev(x), dev(ei), dev(tar), dev(lu), dev(et)), ref) < LOGIT_BAR


def test_one_adam_step_in_the_reference_s_loop_shape(monkeypatch):
    import sys

    import tgm_amd

    monkeypatch.setitem(sys.modules, 'tgm', tgm_amd)
    monkeypatch.setitem(sys.modules, 'tgm.nn', tgm_amd.nn)
    from tgm.nn import NCNPredictor

    meta, a = load('g34_ncn8_triangle_decay')
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    m = NCNPredictor(meta['C'], meta['H'], 1, k=8, cn_time_decay=True).to(DEV).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    before = m.xsmlp[0].weight.detach().clone()
    pos, neg = m(x, ei, tar, lu, et), m(x, ei, tar.flip(0), lu, et)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + torch.nn.functional.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert not torch.equal(before, m.xsmlp[0].weight) and m.xslin.weight.grad is None
    with torch.no_grad():  # the native call sees the updated weights
        sd = {n: v.cpu() for n, v in m.state_dict().items()}
        assert nr.rel_err(m.eval()(x, ei, tar, lu, et), n8.forward(sd, x.cpu(), ei.cpu(), tar.cpu(), lu.cpu(), et.cpu())) < LOGIT_BAR


def test_end_to_end_stream_at_the_example_s_shape():
    """The k = 8 twin of test_ncn_gpu.py's stream test: sampler -> DeduplicationHook -> sampled_edge_list -> TGNMemory ->
    GraphAttentionEmbedding -> NCNPredictor(k=8), a positive and a negative call per batch, then five one-vs-many calls through ONE prepared
    adjacency; the decoder is held to the float64 restatement evaluated on the device's own z."""
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import DeduplicationHook, HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook
    from tgm_amd.nn import GraphAttentionEmbedding, IdentityMessage, LastAggregator, NCNPredictor, TGNMemory, sampled_edge_list
    from tgm_amd.nn.ncn import adjacency
    from tgm_amd.synth import make_stream

    torch.manual_seed(3)
    D, M, T_ = 172, 100, 100
    s = make_stream('wiki', seed=5, num_edges=600, edge_dim=D, n_src=300, n_dst=100, t_hi=600 * 20)
    N = s.num_nodes
    dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1).int(), s.edge_x), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(low=300, high=N, seed=4))
    hm.register('k', RecencyNeighborHook(N, [10], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    hm.register('k', DeduplicationHook(seed_nodes_keys=['neg', 'nbr_nids']))
    mem = TGNMemory(N, D, M, T_, IdentityMessage(D, M, T_), LastAggregator()).to(DEV).train()
    enc = GraphAttentionEmbedding(M, 100, D, mem.time_enc).to(DEV).eval()
    decoder = NCNPredictor(100, 100, 1, k=8, cn_time_decay=True).to(DEV).eval()
    sd = {n: v.cpu() for n, v in decoder.state_dict().items()}
    batches = 0
    with hm.activate('k'), torch.no_grad():
        for batch in DGDataLoader(dg, batch_size=200, hook_manager=hm):
            ei, et, ex = sampled_edge_list(batch)
            z, lu = mem(batch.unique_nids)
            z = enc(z, lu, ei, et, ex)
            loc = lambda ids: batch.global_to_local(ids).long()
            pos = torch.stack([loc(batch.edge_src), loc(batch.edge_dst)])
            neg = torch.stack([loc(batch.edge_src), loc(batch.neg)])
            for what, tar in (('pos', pos), ('neg', neg)):
                out = decoder(z, ei, tar, lu, batch.edge_time)
                ref = n8.forward(sd, z, ei, tar, lu, batch.edge_time)
                e = nr.rel_err(out, ref)
                print(f'k=8 batch {batches} {what}: E={ei.shape[1]} N={z.shape[0]} HIP vs float64 {e:.3e}')
                assert out.shape == (200,) and e < LOGIT_BAR
            adj = adjacency(z.shape[0], ei)
            for p in range(5):  # the evaluation loop: positive p against 20 candidates
                cand = torch.cat([pos[1, p : p + 1], neg[1, :20]])
                tar = torch.stack([pos[0, p].repeat(21), cand])
                t = batch.edge_time[p].repeat(21)
                out = decoder(z, adj, tar, lu, t)
                assert torch.equal(out, decoder(z, ei, tar, lu, t))
                assert nr.rel_err(out, n8.forward(sd, z, ei, tar, lu, t)) < LOGIT_BAR
            mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_x)
            batches += 1
    assert batches == 3


# ---- the reference's own tests (test/unit/test_nn/test_ncn.py) at k = 8, tensors on the device ----------------------------------------------
@pytest.mark.parametrize('cn_time_decay', [True, False])
@pytest.mark.parametrize('train', [True, False])
def test_reference_test_ncn(cn_time_decay, train):
    from tgm_amd.nn import NCNPredictor

    B, D, Z = 2, 5, 1
    ncn = NCNPredictor(in_channels=D, hidden_dim=Z, out_channels=Z, k=8, cn_time_decay=cn_time_decay).to(DEV).train(train)
    node_feat = torch.rand((B, D), device=DEV)
    edge_index = torch.randint(0, B, size=(B, 2), device=DEV)
    edge_time = torch.randint(0, B, size=(B,), device=DEV)
    last_update = torch.zeros(size=(B,), device=DEV)
    h = ncn(node_feat, edge_index, edge_index, last_update, edge_time)
    assert h.shape[0] == B
    assert not torch.isnan(h).any()
    with torch.no_grad():
        assert nr.rel_err(ncn(node_feat, edge_index, edge_index, last_update, edge_time), h) < LOGIT_BAR  # the native and the composed path


def test_reference_test_missing_time_info():
    from tgm_amd.nn import NCNPredictor

    B, D, Z = 2, 5, 1
    ncn = NCNPredictor(in_channels=D, hidden_dim=Z, out_channels=Z, k=8, cn_time_decay=True).to(DEV)
    node_feat = torch.rand((B, D), device=DEV)
    edge_index = torch.randint(0, B, size=(B, 2), device=DEV)
    with pytest.raises(RuntimeError):
        ncn(node_feat, edge_index, edge_index)
    assert ncn(node_feat, edge_index, edge_index, torch.zeros(B, device=DEV), torch.zeros(B, dtype=torch.long, device=DEV)).shape == (B,)


def test_reference_test_bad_init():
    from tgm_amd.nn import NCNPredictor

    with pytest.raises(ValueError):
        NCNPredictor(in_channels=5, hidden_dim=1, out_channels=1, k=16)
    assert NCNPredictor(5, 1, 1, k=8).to(DEV).eval()(torch.rand((2, 5), device=DEV), torch.zeros((2, 1), dtype=torch.long, device=DEV),
                                                    torch.zeros((2, 2), dtype=torch.long, device=DEV)).shape == (2,)  # fmt: skip
