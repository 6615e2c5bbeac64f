"""NCNPredictor on the device: the native call against the reference fixtures and the float64 restatement (degenerate shapes, duplicate
targets, self-loops, a hub row longer than a wave, channel widths, the time-decay corners), strided / int32 edge lists, determinism, the
prepared adjacency, 'all' against 'last', the discarded ReLU, the training path's gradients and an end-to-end stream at the example's shape.

Every parity test prints HIP's distance from float64 (max |got - ref| / max(1, |ref|)) next to the reference's own float32 distance and their
ratio; the measured figures are in DESIGN.md 3.7.
"""
import pytest
import torch

from golden_util import load
import ncn_restate as nr
from test_ncn_cpu import CASES, CN_BAR, LOGIT_BAR, NOISE, SMALL_CASES, build_model, fixture_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RATIO = 2.0  # HIP's distance from float64 over the reference's own float32 distance from float64
NOISE_FLOOR = 1e-7  # below this the reference's sums are exact (one integer-weighted term) and the ratio says nothing


def dev(t):
    return None if t is None else t.to(DEV)


def model_from_fixture(meta, a, **kw):
    m = build_model(meta, **kw)
    sd = nr.fixture_state_dict(meta, a)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd


def run(m, x, ei, tar, lu, et):
    with torch.no_grad():
        return m.get_cn_emb(x, ei, tar, (lu, et)), m(x, ei, tar, lu, et)


def check_against_float64(name, what, got, ref64, noise, bar):
    e = nr.rel_err(got, ref64)
    print(f'{name} {what}: HIP vs float64 {e:.3e}, reference float32 vs float64 {noise:.3e}, ratio {e / noise if noise else float("inf"):.2f}')
    assert e < bar
    if noise >= NOISE_FLOOR:
        assert e <= RATIO * noise
    return e


@pytest.mark.parametrize('N,k', [(1, 2), (1, 4), (5, 2), (5, 4)])
def test_degenerate_shapes(N, k):
    from tgm_amd.nn import NCNPredictor

    torch.manual_seed(N + k)
    m = NCNPredictor(1, 3, 1, k=k).to(DEV).eval()
    x = torch.randn(N, 1, device=DEV)
    ei = torch.zeros((2, 0), dtype=torch.long, device=DEV)
    tar = torch.tensor([[0], [N - 1]], device=DEV)
    cn, out = run(m, x, ei, tar, None, None)
    assert cn.shape == (1, k - 1) and not cn.any()
    sd = {n: v.cpu() for n, v in m.state_dict().items()}
    assert nr.rel_err(out, nr.forward(sd, x, ei, tar, k)) < 1e-6
    with torch.no_grad():
        assert m(x, ei, torch.zeros((2, 0), dtype=torch.long, device=DEV)).shape == (0,)


@pytest.mark.parametrize('name', [c for c in CASES if 'example' not in c])
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
    check_against_float64(name, 'cn_emb', cn, nr.cn_emb(x, ei, tar, meta['k'], lu, et), NOISE[name]['cn_emb'], CN_BAR)
    check_against_float64(name, 'logits', out, nr.forward(sd, x, ei, tar, meta['k'], lu, et), NOISE[name]['logits'], LOGIT_BAR)
    assert nr.rel_err(cn, torch.from_numpy(a['cn_emb'])) < CN_BAR and nr.rel_err(out, torch.from_numpy(a['logits'])) < LOGIT_BAR


def test_hub_row_is_longer_than_a_wave():
    meta, a = load('g18_ncn_hub_k4')
    ei, tar = torch.from_numpy(a['edge_index']), torch.from_numpy(a['tar_ei'])
    deg = torch.bincount(ei.reshape(-1), minlength=meta['N'])
    assert deg[0] > 600 and (tar == 0).all(dim=0).any() and (deg[tar[1]] == 0).any()  # a hub, a (hub, hub) pair, an isolated target


def test_time_decay_corners():
    meta, a = load('g18_ncn_decay_edges')
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    W = nr.decay_weights(lu, et)
    assert (W == 0).any() and (W == 1).any() and (W > 1).any()  # underflow to exactly 0, gaps of 0, a negative gap
    m, _ = model_from_fixture(meta, a)
    cn, _ = run(m, dev(x), dev(ei), dev(tar), dev(lu), dev(et))
    assert nr.rel_err(cn, nr.cn_emb(x, ei, tar, 4, lu, et)) < CN_BAR
    assert nr.rel_err(cn, nr.cn_emb(x, ei, tar, 4)) > 1e-3  # ... and the weights do matter here


@pytest.mark.parametrize('name', ['g18_ncn_rand_k4_decay', 'g18_ncn_hub_k2'])
def test_strided_and_int32_edge_lists_give_the_same_bits(name):
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    E = ei.shape[1]
    base = run(m, x, ei.contiguous(), tar, lu, et)
    buf = torch.full((2, E + 37), 10**6, dtype=torch.long, device=DEV)  # what lies behind the view is never a valid id
    buf[:, :E] = ei
    view = buf[:, :E]
    assert not view.is_contiguous()
    for variant in (view, ei.int(), buf.int()[:, :E], reordered(ei)):
        got = run(m, x, variant, tar, lu, et)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    got = run(m, x, ei, tar.int(), lu, et)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


def reordered(ei):
    """The same edges in another order: the adjacency, and so every bit of the result, does not depend on it."""
    return ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0)).to(ei.device)].flip(0)


@pytest.mark.parametrize('name', ['g18_ncn_onevsmany_k4_decay', 'g18_ncn_hub_k4'])
def test_prepared_adjacency_is_bit_identical_and_reusable(name):
    from tgm_amd.nn.ncn import adjacency

    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    adj = adjacency(meta['N'], ei)
    assert adj.num_nodes == meta['N'] and adj.num_edges == ei.shape[1] and adj.indptr.device.type == 'cuda'
    ip, cols = adj.indptr.cpu().long(), adj.cols.cpu().long()
    A = nr.dense_adjacency(meta['N'], ei.cpu())
    for r in (0, 1, meta['N'] - 1):
        row = cols[ip[r] : ip[r + 1]]
        assert torch.equal(row, row.sort().values) and torch.equal(torch.bincount(row, minlength=meta['N']).double(), A[r])
    assert int(ip[-1]) == 2 * ei.shape[1]
    base = run(m, x, ei, tar, lu, et)
    for _ in range(21):
        got = run(m, x, adj, tar, lu, et)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    with pytest.raises(ValueError, match='prepared adjacency'):
        run(m, x[:-1], adj, tar, lu, et)


def test_all_equals_last_on_single_pairs():
    meta, a = load('g18_ncn_example_k4')
    x, ei, _, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    m_all, sd = model_from_fixture(meta, a, duplicate_targets='all')
    m_last, _ = model_from_fixture(meta, a)
    from tgm_amd.nn.ncn import adjacency

    adj = adjacency(meta['N'], ei)
    src = 8  # shares neighbours with six of the 21 candidates
    tar = torch.stack([torch.full((21,), src, device=DEV), torch.arange(200, 221, device=DEV)])  # one-vs-many
    t = et[:1].repeat(21)
    cn_all, out_all = run(m_all, x, adj, tar, lu, t)
    cn_last, _ = run(m_last, x, adj, tar, lu, t)
    assert not cn_last[:-1, 2 * meta['C'] :].any() and cn_all[:, 2 * meta['C'] :].any(dim=1).sum() > 3
    for r in range(21):
        cn1, out1 = run(m_last, x, adj, tar[:, r : r + 1], lu, t[:1])
        assert torch.equal(cn1[0], cn_all[r]) and torch.equal(out1, out_all[r : r + 1]), r
    ref = nr.forward(sd, x, ei, tar, 4, lu, t, duplicate_targets='all')
    assert nr.rel_err(out_all, ref) < LOGIT_BAR


def test_the_reference_s_relu_is_a_no_op():
    meta, a = load('g18_ncn_rand_k2_plain')
    m, sd = model_from_fixture(meta, a)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    assert (x[tar[0]] * x[tar[1]] < 0).any()
    _, out = run(m, dev(x), dev(ei), dev(tar), None, None)
    assert nr.rel_err(out, nr.forward(sd, x, ei, tar, 2)) < LOGIT_BAR
    assert nr.rel_err(out, nr.forward(sd, x, ei, tar, 2, relu_xs=True)) > 1e-3


@pytest.mark.parametrize('name', ['g18_ncn_rand_k4_plain', 'g18_ncn_rand_k2_decay'])
def test_targets_outside_the_node_table_give_zero_rows_on_both_paths(name):
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    bad = tar.clone()
    bad[0, 2], bad[1, 5] = meta['N'], -1
    W = meta['k'] * meta['C']
    with torch.no_grad():
        xs = m._native_xs(m._inputs(x, ei, bad, lu, et), mlp=False)[0][:, :W].clone()
        out = m(x, ei, bad, lu, et)
    assert not xs[2].any() and not xs[5].any() and xs[0].any()
    # the other rows are what the call without the two pairs gives: an id outside the table marks no last occurrence
    rest = [r for r in range(tar.shape[1]) if r not in (2, 5)]
    with torch.no_grad():
        xs_rest = m._native_xs(m._inputs(x, ei, bad[:, rest], lu, et[rest] if et is not None else None), mlp=False)[0][:, :W]
    assert torch.equal(xs[rest], xs_rest)
    m.train()  # the composed path: the same rows, no device-side assert
    composed = m._torch_xs(m._inputs(x, ei, bad, lu, et))
    assert not composed[2].any() and not composed[5].any() and nr.rel_err(composed, xs) < CN_BAR
    assert nr.rel_err(m(x, ei, bad, lu, et), out) < LOGIT_BAR


@pytest.mark.parametrize('name', ['g18_ncn_rand_k4_decay', 'g18_ncn_hub_k2'])
def test_edges_with_an_endpoint_outside_the_node_table_are_left_out(name):
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    N = meta['N']
    extra = torch.tensor([[N, 0, -1, 2**31 - 1], [1, N + 5, 3, 0]], device=DEV)
    more = torch.cat([extra[:, :2], ei, extra[:, 2:]], dim=1)
    base, got = run(m, x, ei, tar, lu, et), run(m, x, more, tar, lu, et)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    from tgm_amd.nn.ncn import adjacency

    adj, adj0 = adjacency(N, more), adjacency(N, ei)
    assert torch.equal(adj.indptr, adj0.indptr) and torch.equal(adj.cols[: 2 * ei.shape[1]], adj0.cols[: 2 * ei.shape[1]])
    m.train()
    assert nr.rel_err(m._torch_xs(m._inputs(x, more, tar, lu, et)), m._torch_xs(m._inputs(x, ei, tar, lu, et))) == 0.0
    # the composed path through the prepared adjacency walks all 2 E slots, the eight dropped ones behind the last row included
    assert nr.rel_err(m._torch_xs(m._inputs(x, adj, tar, lu, et)), m._torch_xs(m._inputs(x, ei, tar, lu, et))) == 0.0


def test_overlapping_and_expanded_edge_views_are_copied_not_refused():
    meta, a = load('g18_ncn_rand_k2_plain')
    m, _ = model_from_fixture(meta, a)
    x, ei, tar, _, _ = (dev(t) for t in fixture_inputs(meta, a))
    row = ei[0].contiguous()
    both = row.unsqueeze(0).expand(2, -1)  # stride(0) = 0: every edge a self-loop
    overlap = torch.as_strided(ei.reshape(-1).contiguous(), (2, ei.shape[1]), (3, 1))  # rows three entries apart
    for view in (both, overlap):
        assert view.stride(0) < view.shape[1]
        got, want = run(m, x, view, tar, None, None), run(m, x, view.contiguous(), tar, None, None)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize('name', ['g18_ncn_selfloop_k4_decay', 'g18_ncn_bothways_k2_plain', 'g18_ncn_hub_k4'])
def test_training_path_gradients(name):
    meta, a = load(name)
    m, _ = model_from_fixture(meta, a)
    m.train()
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    xd = dev(x).requires_grad_(True)
    out = m(xd, dev(ei), dev(tar), dev(lu), dev(et))
    assert out.requires_grad
    wts = torch.linspace(-1, 1, out.numel(), dtype=torch.float64)
    (out * wts.to(DEV).float()).sum().backward()
    sd = {n: v.detach().cpu().double().requires_grad_(True) for n, v in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    ref = nr.forward(sd, x64, ei, tar, meta['k'], lu, et)
    assert nr.rel_err(out, ref) < LOGIT_BAR
    (ref * wts).sum().backward()
    bar = lambda g: 1e-4 * float(g.abs().max())  # the project's gradient bar: 1e-4 of each gradient's max
    assert float((xd.grad.cpu().double() - x64.grad).abs().max()) <= bar(x64.grad)
    for n, p in m.named_parameters():
        if n.startswith('xslin'):
            assert p.grad is None and sd[n].grad is None  # unused in forward
        else:
            assert float((p.grad.cpu().double() - sd[n].grad).abs().max()) <= bar(sd[n].grad), n
    with torch.no_grad():  # the same weights through the native call
        assert nr.rel_err(m.eval()(dev(x), dev(ei), dev(tar), dev(lu), dev(et)), ref) < LOGIT_BAR


def test_one_adam_step_in_the_reference_s_loop_shape(monkeypatch):
    import sys

    import tgm_amd

    monkeypatch.setitem(sys.modules, 'tgm', tgm_amd)
    monkeypatch.setitem(sys.modules, 'tgm.nn', tgm_amd.nn)
    from tgm.nn import NCNPredictor

    meta, a = load('g18_ncn_rand_k4_decay')
    x, ei, tar, lu, et = (dev(t) for t in fixture_inputs(meta, a))
    m = NCNPredictor(meta['C'], meta['H'], 1, k=4, cn_time_decay=True).to(DEV).train()
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
        assert nr.rel_err(m.eval()(x, ei, tar, lu, et), nr.forward(sd, x, ei, tar, 4, lu, et)) < LOGIT_BAR


@pytest.mark.parametrize('name', ['g18_ncn_example_k2', 'g18_ncn_example_k4'])
def test_example_shape_fixture(name):
    meta, a = load(name)
    m, sd = model_from_fixture(meta, a)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    cn, out = run(m, dev(x), dev(ei), dev(tar), dev(lu), dev(et))
    check_against_float64(name, 'cn_emb', cn, nr.cn_emb(x, ei, tar, meta['k'], lu, et), NOISE[name]['cn_emb'], CN_BAR)
    check_against_float64(name, 'logits', out, nr.forward(sd, x, ei, tar, meta['k'], lu, et), NOISE[name]['logits'], LOGIT_BAR)
    assert nr.rel_err(out, torch.from_numpy(a['logits'])) < LOGIT_BAR


@pytest.mark.parametrize('k', [2, 4])
def test_end_to_end_stream_at_the_example_s_shape(k):
    """Sampler -> DeduplicationHook -> sampled_edge_list -> TGNMemory -> GraphAttentionEmbedding -> NCNPredictor (a positive and a negative
    call per batch), then the evaluation loop's one-vs-many calls through ONE prepared adjacency; the decoder is held to the float64
    restatement evaluated on the device's own z."""
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
    decoder = NCNPredictor(100, 100, 1, k=k, cn_time_decay=True).to(DEV).eval()
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
                ref = nr.forward(sd, z, ei, tar, k, lu, batch.edge_time)
                e = nr.rel_err(out, ref)
                print(f'k={k} batch {batches} {what}: E={ei.shape[1]} N={z.shape[0]} HIP vs float64 {e:.3e}')
                assert out.shape == (200,) and e < LOGIT_BAR
            adj = adjacency(z.shape[0], ei)
            for p in range(5):  # the evaluation loop: positive p against 20 candidates
                cand = torch.cat([pos[1, p : p + 1], neg[1, :20]])
                tar = torch.stack([pos[0, p].repeat(21), cand])
                t = batch.edge_time[p].repeat(21)
                out = decoder(z, adj, tar, lu, t)
                assert torch.equal(out, decoder(z, ei, tar, lu, t))
                assert nr.rel_err(out, nr.forward(sd, z, ei, tar, k, lu, t)) < LOGIT_BAR
            mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_x)
            batches += 1
    assert batches == 3
