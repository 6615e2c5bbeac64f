"""ROLAND / sparse GCNConv without a GPU: the restatement (tests/roland_restate.py) against the reference's recorded embeddings
(tests/golden/g24_roland_*.npz) and against a dense-matrix evaluation, the Python surface (constructor, state_dict, import paths), the
composed path on the CPU, the module's state handling, the ABI additions and the refusal to compute off the GPU."""
import ctypes
import inspect

import pytest
import torch

import roland_restate as rr


def make_model(meta, params, **kw):
    from tgm_amd.nn import ROLAND

    model = ROLAND(meta['input_channel'], meta['out_channel'], meta['num_nodes'], update=meta['update'], tau=meta['tau'] if meta['update'] is None else 0.5, **kw)
    model.load_state_dict(params, strict=True)
    return model


def test_fixture_set_is_complete():
    assert rr.fixture_names() == rr.EXPECTED_FIXTURES


@pytest.mark.parametrize('name', rr.EXPECTED_FIXTURES)
def test_restatement_reproduces_the_reference_embeddings(name):
    meta, params, snaps = rr.load_fixture(name)
    assert 3 <= len(snaps) <= 4 and meta['num_nodes'] <= 30
    for dtype in (torch.float32, torch.float64):
        for s, (h0, h1) in rr.restated_replay(meta, params, snaps, dtype):
            rr.close(h0.float(), snaps[s]['H0'], f'{name} H0 {s} {dtype}')
            rr.close(h1.float(), snaps[s]['H1'], f'{name} H1 {s} {dtype}')


def test_fixtures_hold_what_their_names_say():
    meta, params, _ = rr.load_fixture('learnable')
    assert meta['update'] == 'learnable' and params['tau'].item() == pytest.approx(0.3)
    assert rr.load_fixture('learnable_default')[1]['tau'].item() == 0.0
    meta, _, snaps = rr.load_fixture('moving')
    assert meta['update'] == 'moving' and snaps[0]['counts'] == (None, None)
    assert len({c['counts'][1] / sum(c['counts']) for c in snaps[1:]}) == len(snaps) - 1
    meta, _, _ = rr.load_fixture('fixed_tau')
    assert meta['update'] is None and meta['tau'] == 0.7
    assert [rr.load_fixture(n)[0]['update'] for n in ('gru', 'mlp')] == ['gru', 'mlp']
    meta, _, snaps = rr.load_fixture('loops_dups_isolated')
    for s in snaps:
        ei = s['edge_index']
        pairs = list(map(tuple, ei.t().tolist()))
        loops = [a for a, b in pairs if a == b]
        assert max(loops.count(v) for v in set(loops)) >= 3 and len(set(pairs)) < len(pairs)  # several loops on one node, repeats
        assert set(range(meta['num_nodes'])) - set(ei[1].tolist())  # nodes without in-edges
    assert [s['edge_index'].shape[1] > 0 for s in rr.load_fixture('empty_snapshot')[2]] == [True, False, True]
    meta, _, _ = rr.load_fixture('odd_widths')
    assert meta['input_channel'] != meta['out_channel'] and meta['input_channel'] % 4 and meta['out_channel'] % 4


# a 7-node graph: a two-way pair, a chain, a repeated edge, two self loops on node 4 and one on node 0, a node that only receives, an isolated node
EI7 = torch.tensor([[0, 1, 1, 2, 3, 3, 4, 4, 0, 4, 0], [1, 0, 2, 3, 4, 4, 4, 5, 5, 4, 0]])
W7 = torch.tensor([0.5, 1.5, 2.0, 0.7, 1.1, 0.4, 3.0, 0.9, 1.3, 0.25, 1.75], dtype=torch.float64)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('fill,add_self_loops', [(1.0, True), (2.0, True), (1.0, False)])
def test_restated_gcn_norm_is_what_the_definition_says(weighted, fill, add_self_loops):
    w = W7 if weighted else None
    norm = rr.gcn_norm(EI7, w, 7, fill, add_self_loops)
    A = rr.dense_adjacency(norm, 7)
    # by hand: the dense matrix of A (+ loops), degrees over the destination
    M = torch.zeros(7, 7, dtype=torch.float64)
    ww = torch.ones(11, dtype=torch.float64) if w is None else w
    for e in range(11):
        s, d = int(EI7[0, e]), int(EI7[1, e])
        if s == d and add_self_loops:
            M[d, d] = ww[e]  # the last loop wins
        else:
            M[d, s] += ww[e]
    if add_self_loops:
        for i in range(7):
            if M[i, i] == 0:
                M[i, i] = fill
    deg = M.sum(1)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    assert torch.allclose(A, dinv[:, None] * M * dinv[None, :], atol=1e-14)
    if add_self_loops and weighted:
        assert norm[3][4].item() == pytest.approx(0.25 / (1.1 + 0.4 + 0.25))  # node 4: the loop at the highest edge position, 0.25, not 3.0
    if not add_self_loops:
        assert not norm[3].any() and deg[6] == 0 and not A[6].any()
    x = torch.randn(7, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert rr.rel_err(rr.propagate(norm, x), A @ x) < 1e-14


def test_import_paths_and_signatures():
    import tgm_amd.nn.encoder.roland as mod
    import tgm_amd.nn.roland
    from tgm_amd.nn import ROLAND as A
    from tgm_amd.nn import GCNConv
    from tgm_amd.nn.encoder import ROLAND

    assert mod is tgm_amd.nn.roland and mod.ROLAND is ROLAND is A
    sig = inspect.signature(ROLAND.__init__)
    assert list(sig.parameters)[1:] == ['input_channel', 'out_channel', 'num_nodes', 'dropout', 'update', 'tau']
    assert [sig.parameters[k].default for k in ('dropout', 'update', 'tau')] == [0.0, 'learnable', 0.5]
    assert list(inspect.signature(ROLAND.forward).parameters)[1:] == ['node_x', 'edge_index', 'previous_embeddings', 'num_current_edges', 'num_previous_edges']
    model = ROLAND(input_channel=256, out_channel=256, num_nodes=40, dropout=0.1, update='learnable')  # examples/linkproppred/roland.py
    assert isinstance(model.conv1, GCNConv) and isinstance(model.conv2, GCNConv)
    assert [tuple(t.shape) for t in model.previous_embeddings] == [(40, 256)] * 2 and not any(t.any() for t in model.previous_embeddings)
    with pytest.raises(AssertionError):
        ROLAND(4, 4, 5, update='bogus')
    with pytest.raises(AssertionError):
        ROLAND(4, 4, 5, update=None, tau=1.5)
    assert ROLAND(4, 4, 5, update='moving').tau.item() == 0.0 and ROLAND(4, 4, 5, update=None, tau=0.25).tau.item() == 0.25


@pytest.mark.parametrize('update', ['moving', 'learnable', 'gru', 'mlp', None])
def test_state_dict_keys_per_update_mode(update):
    from tgm_amd.nn import ROLAND

    model = ROLAND(6, 8, 20, update=update)
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == rr.expected_shapes(6, 8, update)
    if update == 'learnable':
        assert isinstance(model.tau, torch.nn.Parameter) and sd['tau'].item() == 0.0
    # reset_parameters resets the two convolutions only
    before = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        model.conv1.bias.fill_(1.0)
    model.reset_parameters()
    after = model.state_dict()
    assert not after['conv1.bias'].any() and not torch.equal(after['conv1.lin.weight'], before['conv1.lin.weight'])
    assert all(torch.equal(after[k], before[k]) for k in after if not k.startswith('conv'))


@pytest.mark.parametrize('name', rr.EXPECTED_FIXTURES)
def test_state_dict_keys_equal_the_fixture_s(name):
    meta, params, _ = rr.load_fixture(name)
    sd = make_model(meta, params).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}


@pytest.mark.parametrize('name', rr.EXPECTED_FIXTURES)
def test_composed_path_is_the_restated_arithmetic(name):
    """ROLAND.forward_composed (device-agnostic torch ops), float32 on the CPU, as a recurrence, against the float64 restatement."""
    meta, params, snaps = rr.load_fixture(name)
    model = make_model(meta, params).eval()
    ref = rr.restated_replay(meta, params, snaps)
    got = list(rr.replay(meta, snaps, lambda s, x, ei, prev, cur, prv: model.forward_composed(x, ei.to(torch.int32), prev, cur, prv)))
    for s, out in got:
        for l in range(2):
            assert not out[l].requires_grad and out[l].dtype == torch.float32
            assert rr.rel_err(out[l], ref[s][1][l]) < 5e-6, (name, s, l)
            rr.close(out[l], snaps[s][f'H{l}'], f'{name} H{l} {s}')


def test_composed_path_skips_out_of_range_edges_and_keeps_its_state():
    from tgm_amd.nn import ROLAND

    torch.manual_seed(3)
    model = ROLAND(4, 3, 7, update=None, tau=0.25).eval()
    x = torch.randn(7, 4)
    ei = EI7
    a = model.forward_composed(x, ei)
    b = model.forward_composed(x, torch.cat([ei, torch.tensor([[2, -1], [9, 3]])], dim=1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # passed embeddings are copied: overwriting the caller's tensors afterwards does not change a later call without them
    prev = [torch.randn(7, 3), torch.randn(7, 3)]
    c = model.forward_composed(x, ei, prev)
    prev[0].zero_(), prev[1].zero_()
    d = model.forward_composed(x, ei)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and not torch.equal(a[1], c[1])
    # the forward does not store its own outputs
    assert not torch.equal(model.previous_embeddings[1], d[1])
    with pytest.raises(ValueError):
        model.forward_composed(torch.randn(6, 4), ei.clamp(max=5))


def test_dropout_in_training_is_seeded_and_detached():
    from tgm_amd.nn import ROLAND

    model = ROLAND(4, 8, 7, dropout=0.5, update='gru').train()
    x = torch.randn(7, 4)
    torch.manual_seed(1)
    a = model.forward_composed(x, EI7)
    torch.manual_seed(1)
    b = model.forward_composed(x, EI7)
    c = model.forward_composed(x, EI7)
    assert torch.equal(a[1], b[1]) and not torch.equal(a[1], c[1]) and not a[1].requires_grad and torch.isfinite(a[1]).all()


def test_no_cpu_fallback():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import ROLAND

    for update in ('learnable', 'gru'):
        model = ROLAND(4, 3, 7, update=update).eval()
        with pytest.raises(NativeLibraryError):
            model(torch.randn(7, 4), EI7)
        with torch.no_grad(), pytest.raises(NativeLibraryError):
            model(torch.randn(7, 4), EI7)
    with pytest.raises(NativeLibraryError):
        ROLAND(4, 3, 7, dropout=0.5).train()(torch.randn(7, 4), EI7)


def test_abi_additions():
    from tgm_amd import _native

    lib = _native.load()
    for name in ('tgmx_gcn_workspace_bytes', 'tgmx_gcn_norm_csr', 'tgmx_gcn_propagate', 'tgmx_roland_forward'):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.tgmx_abi_sizeof(26) == ctypes.sizeof(_native.RolandFwd) > 0
    assert _native.GCN_EPI == {'none': 0, 'relu': 1, 'tau': 2}
    assert _native.ROLAND_UPDATE == {'moving': 0, 'learnable': 0, None: 0, 'mlp': 1, 'gru': 2}
    assert lib.tgmx_gcn_workspace_bytes(0, 1) > 0 and lib.tgmx_gcn_workspace_bytes(-1, 5) == 0 and lib.tgmx_gcn_workspace_bytes(5, 0) == 0
