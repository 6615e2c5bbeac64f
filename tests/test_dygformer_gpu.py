"""DyGFormer on the device: co-occurrence counts bit for bit, the co-occurrence encoder, the transformer layer and the whole encoder
against the reference fixtures and the float64 restatement (the ceiling, and the ratio to the reference's own float32 distance), the
one-call forward against its launch-by-launch twin, encode_pairs against forward on gathered tensors, the composed path outside the
native envelope, the training path's gradients, and a reference-style training / evaluation step.

Measured on an MI355X (max |got - ref| / max(1, |ref|) against float64; the reference's own float32 distance in brackets): see DESIGN.md 3.5.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_util import load
import dygformer_restate as dr
from test_dygformer_cpu import COUNT_CASES, ENCODER_CASES, LAYER_CASES, NOISE, encoder_inputs, fixture_state_dict, restated

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4  # the ceiling (tests/test_graphmixer_gpu.py's), asserted where the time gaps stay below 1e5
RATIO = 2.0  # HIP's distance from float64 over the reference's own float32 distance from float64


def counts_on_device(s, d):
    from tgm_amd.nn import NeighborCooccurrenceEncoder

    enc = NeighborCooccurrenceEncoder(4, DEV)
    fs, fd = enc._count_nodes_freq(torch.as_tensor(s).to(DEV), torch.as_tensor(d).to(DEV))
    return fs.cpu().numpy().astype(np.int64), fd.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize('name', COUNT_CASES)
def test_counts_match_the_reference_fixture_bit_for_bit(name):
    _, a = load(name)
    cs, cd = counts_on_device(a['src_seq'], a['dst_seq'])
    assert np.array_equal(cs, a['src_counts']) and np.array_equal(cd, a['dst_counts'])


@pytest.mark.parametrize('L,N,P', [(2, 2, 50), (3, 1, 9), (33, 4, 40), (64, 9, 30), (257, 20, 11), (1000, 3, 5), (2048, 50, 6), (2048, 2, 3)])
def test_counts_match_the_restatement_on_random_sequences(L, N, P):
    rng = np.random.default_rng(L * 7 + N)
    s, d = rng.integers(0, N, (P, L)).astype(np.int32), rng.integers(0, N, (P, L)).astype(np.int32)
    for a in (s, d):
        a[:, 1:][rng.random((P, L - 1)) < 0.3] = -1
    s[0, 1:] = -1
    d[1] = s[1]
    cs, cd = counts_on_device(s, d)
    ws, wd = dr.cooccurrence_counts(s, d)
    assert np.array_equal(cs, ws) and np.array_equal(cd, wd)


def test_cooccurrence_encoder_matches_the_reference_fixture():
    from tgm_amd.nn import NeighborCooccurrenceEncoder

    meta, a = load('g16_dygformer_cooc')
    enc = NeighborCooccurrenceEncoder(meta['feat_dim'], 'cpu')
    enc.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')}, strict=True)
    enc = enc.to(DEV).eval()
    with torch.no_grad():
        fs, fd = enc(torch.from_numpy(a['src_seq']).to(DEV), torch.from_numpy(a['dst_seq']).to(DEV))
    # the count table keeps the reference's per-element arithmetic: a C-term float32 contraction plus two adds, (C + 2) 2^-23 at the most
    bar = (meta['feat_dim'] + 2) * 2.0**-23
    sd = {k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')}
    r64 = [dr.cooccurrence_encode(sd, 'neighbor_co_occurrence_encoder.', torch.from_numpy(c)) for c in dr.cooccurrence_counts(a['src_seq'], a['dst_seq'])]
    e64 = max(dr.rel_err(fs, r64[0]), dr.rel_err(fd, r64[1]))
    efix = max(dr.rel_err(fs, torch.from_numpy(a['src_feat'])), dr.rel_err(fd, torch.from_numpy(a['dst_feat'])))
    print(f'g16_dygformer_cooc: HIP vs float64 {e64:.3e} (reference float32: {NOISE["fixtures"]["g16_dygformer_cooc"]:.3e}), vs the fixture {efix:.3e}')
    assert e64 < bar and efix < bar
    gs, gd = enc(torch.from_numpy(a['src_seq']).to(DEV), torch.from_numpy(a['dst_seq']).to(DEV))  # gradients enabled: the composed path
    assert gs.requires_grad and dr.rel_err(gs, fs) < 1e-5 and dr.rel_err(gd, fd) < 1e-5


@pytest.mark.parametrize('name', LAYER_CASES)
def test_transformer_layer_matches_the_reference_fixture(name):
    from tgm_amd.nn import TransformerEncoder

    meta, a = load(name)
    sd = fixture_state_dict(meta, a)
    m = TransformerEncoder(meta['attention_dim'], meta['num_heads'])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    x = torch.from_numpy(a['x'])
    with torch.no_grad():
        y = m(x.to(DEV))
    e64 = dr.rel_err(y, dr.transformer_layer(sd, '', x.double(), meta['num_heads']))
    noise = NOISE['fixtures'][name]
    print(f'{name}: HIP vs float64 {e64:.3e}, reference float32 vs float64 {noise:.3e}, ratio {e64 / noise:.2f}; HIP vs the fixture '
          f'{dr.rel_err(y, torch.from_numpy(a["y"])):.3e}')
    assert e64 < BAR and dr.rel_err(y, torch.from_numpy(a['y'])) < BAR
    assert e64 <= RATIO * noise


@pytest.mark.parametrize('d,H,T,B', [(128, 1, 128, 3), (256, 2, 128, 2), (200, 2, 100, 3), (96, 3, 77, 2), (128, 1, 65, 2)],
                         ids=['T128_dh128', 'T128_dh128_h2', 'T100_dh100', 'T77_dh32', 'T65_dh128'])  # fmt: skip
def test_transformer_layer_upper_half_of_the_native_envelope(d, H, T, B, monkeypatch):
    """More than four score tiles per row tile, T not a multiple of 16, head dimension 128, and the launches past 64 KiB of LDS."""
    from tgm_amd.nn import TransformerEncoder
    from tgm_amd.nn import dygformer as mod

    torch.manual_seed(d + T)
    m = TransformerEncoder(d, H).to(DEV).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
        x = torch.randn(B, T, d, device=DEV) * 1.5 + 0.3
        took_native = []
        orig = mod._native_layer
        monkeypatch.setattr(mod, '_native_layer', lambda *a, **k: took_native.append(1) or orig(*a, **k))
        torch_fwd = m._torch_forward
        monkeypatch.setattr(m, '_torch_forward', lambda *a, **k: took_native.append(0) or torch_fwd(*a, **k))
        y = m(x)
    assert took_native == [1]  # the native layer ran and did not hand over to the composed path
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64 = dr.transformer_layer(sd, '', x.cpu().double(), H)
    r32 = dr.transformer_layer(sd, '', x.cpu(), H)
    e64, n32 = dr.rel_err(y, r64), dr.rel_err(r32, r64)
    print(f'd {d} heads {H} T {T}: HIP vs float64 {e64:.3e}, float32 restatement vs float64 {n32:.3e}, ratio {e64 / n32:.2f}')
    assert e64 < BAR and e64 <= RATIO * n32


def test_encoder_with_128_tokens_per_pair():
    from tgm_amd.nn import DyGFormer

    torch.manual_seed(6)
    b = wiki_batches(E=1600, bs=40, k=63, D=5)[30]
    m = DyGFormer(6, 5, 8, 32, output_dim=7, num_layers=2, num_heads=1, max_input_sequence_length=64, device=DEV).to(DEV).eval()  # dh = 128
    assert m._native_ok(64)
    node_x = torch.randn(400, 6, device=DEV)
    sr, dr_ = pair_rows(b, False)
    nids, nt, nx = gathered(b, sr, dr_)
    with torch.no_grad():
        zs, zd = m(node_x, torch.stack([b.edge_src, b.edge_dst]), b.edge_time, nids, nt, nx)
        cs, cd = m._torch_forward(m._inputs(node_x, b.edge_src, b.edge_dst, b.edge_time, nids, nt, nx, None, None))
    assert not torch.equal(zs, cs)  # the native call, not the composed path
    r64 = cpu_restated(m, node_x, b.edge_src, b.edge_dst, b.edge_time, nids, nt, nx)
    r32 = cpu_restated(m, node_x, b.edge_src, b.edge_dst, b.edge_time, nids, nt, nx, dtype=torch.float32)
    e64 = max(dr.rel_err(zs, r64[0]), dr.rel_err(zd, r64[1]))
    n32 = max(dr.rel_err(r32[0], r64[0]), dr.rel_err(r32[1], r64[1]))
    print(f'128 tokens per pair, dh 128: HIP vs float64 {e64:.3e}, float32 restatement vs float64 {n32:.3e}, ratio {e64 / n32:.2f}')
    assert e64 < BAR and e64 <= RATIO * n32


def model_from_fixture(meta, a):
    from tgm_amd.nn import DyGFormer

    sd = fixture_state_dict(meta, a)
    m = DyGFormer(**meta['dims'])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd


def run_forward(m, i):
    dev = lambda t: t.to(DEV)
    return m(dev(i['node_x']), torch.stack([dev(i['src']), dev(i['dst'])]), dev(i['edge_time']), dev(i['nbr_nids']), dev(i['nbr_time']), dev(i['nbr_edge_x']))


@pytest.mark.parametrize('name', ENCODER_CASES)
def test_encoder_matches_the_reference_fixture(name, monkeypatch):
    meta, a = load(name)
    m, sd = model_from_fixture(meta, a)
    i = encoder_inputs(a)
    with torch.no_grad():
        zs, zd = run_forward(m, i)
        zs2, zd2 = (t.clone() for t in run_forward(m, i))
        monkeypatch.setenv('TGMX_DYGFORMER_PY', '1')
        ts, td = run_forward(m, i)
        monkeypatch.delenv('TGMX_DYGFORMER_PY')
    assert torch.equal(zs, zs2) and torch.equal(zd, zd2)
    assert torch.equal(zs, ts) and torch.equal(zd, td)  # the one call = its launches one by one
    rs, rd = restated(meta, a, sd)
    e64 = max(dr.rel_err(zs, rs), dr.rel_err(zd, rd))
    efix = max(dr.rel_err(zs, torch.from_numpy(a['z_src'])), dr.rel_err(zd, torch.from_numpy(a['z_dst'])))
    noise = NOISE['fixtures'][name]
    print(f'{name}: HIP vs float64 {e64:.3e}, reference float32 vs float64 {noise:.3e}, ratio {e64 / noise:.2f}; HIP vs the fixture {efix:.3e}')
    if meta['max_gap'] <= 10**5:
        assert e64 < BAR and efix < BAR
    else:
        assert efix <= e64 + noise  # bounded by the sum of the two distances, not by the ceiling
    assert e64 <= RATIO * noise


def wiki_batches(E=2400, bs=200, k=31, D=172):
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook
    from tgm_amd.synth import make_stream

    s = make_stream('wiki', seed=5, num_edges=E, edge_dim=D, n_src=300, n_dst=100, t_hi=E * 20)
    dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1).int(), s.edge_x), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=400))
    hm.register('k', RecencyNeighborHook(400, [k], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
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


EXAMPLE = dict(node_feat_dim=128, edge_x_dim=172, time_feat_dim=100, channel_embedding_dim=50, output_dim=172, patch_size=1, num_layers=2,
               num_heads=2, dropout=0.1, max_input_sequence_length=32)  # fmt: skip


def cpu_restated(m, node_x, src, dst, t, nids, nt, nx, dtype=torch.float64):
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    c = lambda v: v.detach().cpu()
    return dr.dygformer_forward(sd, m.patch_size, m.num_layers, m.num_heads, c(node_x), c(src), c(dst), c(t), c(nids), c(nt), c(nx), dtype=dtype)


def test_encoder_end_to_end_on_sampler_output(monkeypatch):
    from tgm_amd.nn import DyGFormer

    torch.manual_seed(0)
    batches = wiki_batches()
    m = DyGFormer(**EXAMPLE, device=DEV).to(DEV).eval()
    node_x = torch.randn(400, 128, device=DEV)
    pad_frac = []
    for j in (0, 1, len(batches) - 1):  # the first batch (empty history: every slot padded), an early one (mostly pads), the last
        b = batches[j]
        pad_frac.append(float((b.nbr_nids[0] == -1).float().mean()))
        for negatives in (False, True):
            sr, dr_ = pair_rows(b, negatives)
            src, dst = b.edge_src, (b.neg if negatives else b.edge_dst)
            nids, nt, nx = gathered(b, sr, dr_)
            with torch.no_grad():
                zs, zd = m(node_x, torch.stack([src, dst]), b.edge_time, nids, nt, nx)
                es, ed = m.encode_pairs(node_x, src, dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr_)
                monkeypatch.setenv('TGMX_DYGFORMER_PY', '1')
                ts, td = m.encode_pairs(node_x, src, dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr_)
                monkeypatch.delenv('TGMX_DYGFORMER_PY')
            assert torch.equal(zs, es) and torch.equal(zd, ed), j  # encode_pairs = forward on gathered tensors
            assert torch.equal(es, ts) and torch.equal(ed, td), j
            r64 = cpu_restated(m, node_x, src, dst, b.edge_time, nids, nt, nx)
            r32 = cpu_restated(m, node_x, src, dst, b.edge_time, nids, nt, nx, dtype=torch.float32)
            e64 = max(dr.rel_err(zs, r64[0]), dr.rel_err(zd, r64[1]))
            n32 = max(dr.rel_err(r32[0], r64[0]), dr.rel_err(r32[1], r64[1]))
            gap = int((b.edge_time[:, None] - b.nbr_edge_time[0][: b.edge_src.numel()]).where(b.nbr_nids[0][: b.edge_src.numel()] != -1, torch.tensor(0, device=DEV)).max())
            print(f'batch {j} negatives={negatives}: HIP vs float64 {e64:.3e}, float32 restatement vs float64 {n32:.3e}, ratio {e64 / n32:.2f}, max gap {gap}')
            if gap < 10**5:
                assert e64 < BAR, j
            assert e64 <= RATIO * n32, j
    assert pad_frac[0] == 1.0 and pad_frac[1] > 0.5


def test_encode_pairs_one_vs_many_equals_forward_on_gathered_tensors():
    from tgm_amd.nn import DyGFormer

    torch.manual_seed(1)
    b = wiki_batches(E=1200, bs=100, k=15, D=12)[6]
    m = DyGFormer(9, 12, 10, 6, output_dim=11, patch_size=4, num_layers=2, num_heads=3, max_input_sequence_length=16, device=DEV).to(DEV).eval()
    node_x = torch.randn(400, 9, device=DEV)
    n, M = b.edge_src.numel(), 7  # every positive source against M destinations drawn from the batch's seeds
    g = torch.Generator().manual_seed(2)
    src_rows = torch.arange(n, dtype=torch.int32).repeat_interleave(M).to(DEV)
    dst_rows = torch.randint(n, 3 * n, (n * M,), generator=g, dtype=torch.int32).to(DEV)
    seeds = torch.cat([b.edge_src, b.edge_dst, b.neg])
    src, dst, t = seeds[src_rows.long()], seeds[dst_rows.long()], b.edge_time.repeat_interleave(M)
    nids, nt, nx = gathered(b, src_rows, dst_rows)
    with torch.no_grad():
        zs, zd = m(node_x, torch.stack([src, dst]), t, nids, nt, nx)
        es, ed = m.encode_pairs(node_x, src, dst, t, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], src_rows, dst_rows)
    assert torch.equal(zs, es) and torch.equal(zd, ed)
    r = cpu_restated(m, node_x, src, dst, t, nids, nt, nx)
    assert max(dr.rel_err(zs, r[0]), dr.rel_err(zd, r[1])) < BAR


@pytest.mark.parametrize('dims', [dict(max_input_sequence_length=136, patch_size=1, channel_embedding_dim=4, num_heads=2),  # 272 tokens per pair
                                  dict(max_input_sequence_length=8, patch_size=2, channel_embedding_dim=33, num_heads=1)],  # head dimension 132
                         ids=['tokens', 'head_dim'])  # fmt: skip
def test_outside_the_native_envelope_the_composed_path_matches_the_restatement(dims):
    from tgm_amd.nn import DyGFormer

    torch.manual_seed(3)
    k = dims['max_input_sequence_length'] - 1
    b = wiki_batches(E=1000, bs=50, k=k, D=5)[8]
    m = DyGFormer(6, 5, 8, output_dim=7, num_layers=1, device=DEV, **dims).to(DEV).eval()
    assert not m._native_ok(k + 1)
    node_x = torch.randn(400, 6, device=DEV)
    sr, dr_ = pair_rows(b, False)
    nids, nt, nx = gathered(b, sr, dr_)
    with torch.no_grad():
        zs, zd = m(node_x, torch.stack([b.edge_src, b.edge_dst]), b.edge_time, nids, nt, nx)
    r = cpu_restated(m, node_x, b.edge_src, b.edge_dst, b.edge_time, nids, nt, nx)
    assert max(dr.rel_err(zs, r[0]), dr.rel_err(zd, r[1])) < BAR


def test_training_path_gradients():
    from tgm_amd.nn import DyGFormer

    torch.manual_seed(4)
    b = wiki_batches(E=1200, bs=100, k=7, D=12)[3]
    m = DyGFormer(4, 12, 8, 6, output_dim=5, patch_size=2, num_layers=2, num_heads=2, dropout=0.0, max_input_sequence_length=8, device=DEV).to(DEV).train()
    node_x = torch.randn(400, 4, device=DEV)
    sr, dr_ = pair_rows(b, True)
    nids, nt, nx = gathered(b, sr, dr_)
    zs, zd = m(node_x, torch.stack([b.edge_src, b.neg]), b.edge_time, nids, nt, nx)
    assert zs.requires_grad
    z = torch.cat([zs, zd])
    (z * torch.linspace(-1, 1, z.numel(), device=DEV).view_as(z)).sum().backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    c = lambda v: v.detach().cpu()
    rs, rd = dr.dygformer_forward(sd, 2, 2, 2, c(node_x), c(b.edge_src), c(b.neg), c(b.edge_time), c(nids), c(nt), c(nx))
    zr = torch.cat([rs, rd])
    assert dr.rel_err(z, zr) < BAR
    (zr * torch.linspace(-1, 1, zr.numel(), dtype=torch.float64).view_as(zr)).sum().backward()
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert dr.rel_err(p.grad, sd[n].grad) < BAR, n
    with torch.no_grad():  # the same weights through the native inference call
        es, ed = m.eval()(node_x, torch.stack([b.edge_src, b.neg]), b.edge_time, nids, nt, nx)
    assert dr.rel_err(torch.cat([es, ed]), zr) < BAR


def test_reference_style_training_and_evaluation_step(monkeypatch):
    """``from tgm.nn import DyGFormer`` with tgm -> tgm_amd: construct, load a reference state_dict, one training and one evaluation step."""
    import sys

    import tgm_amd

    monkeypatch.setitem(sys.modules, 'tgm', tgm_amd)
    monkeypatch.setitem(sys.modules, 'tgm.nn', tgm_amd.nn)
    from tgm.nn import DyGFormer

    meta, a = load('g16_dygformer_small_p2')
    m = DyGFormer(**meta['dims'], device=DEV)
    m.load_state_dict(fixture_state_dict(meta, a), strict=True)
    m = m.to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    i = encoder_inputs(a)
    m.train()
    zs, zd = run_forward(m, i)
    loss = (zs * zd).sum(dim=1).sigmoid().mean()
    loss.backward()
    opt.step()
    m.eval()
    with torch.no_grad():
        es, ed = run_forward(m, i)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    rs, rd = restated(meta, a, sd)
    assert es.shape == zs.shape and max(dr.rel_err(es, rs), dr.rel_err(ed, rd)) < BAR  # the native call sees the updated weights
    assert not torch.equal(es, zs.detach())
