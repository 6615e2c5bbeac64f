"""The decoders without a GPU: the restatement (tests/decoders_restate.py) against the reference's recorded outputs
(tests/golden/g26_decoder_*.npz), the reference's own three test files replayed against ``tgm_amd``, the Python surface (import paths,
signatures, ``state_dict`` keys, the protocol error), the torch path on the host against the restatement, ``score_pairs`` /
``query_one_vs_many`` on the host against the per-positive loop, and the ABI additions."""
import ctypes
import inspect
import os
import subprocess
import sys

import pytest
import torch

import decoders_restate as dr

HERE = os.path.dirname(os.path.abspath(__file__))


def build(meta, sd):
    from tgm_amd.nn import GraphPredictor, LinkPredictor, NodePredictor
    from tgm_amd.nn.modules import ConcatMerge, LearnableSumMerge, MeanEmbdPooling, SumEmbdPooling

    kw, op = meta['kw'], meta['op']
    if meta['kind'] == 'link':
        model = LinkPredictor(**kw, merge_op=(ConcatMerge if op == 'concat' else LearnableSumMerge)(kw['node_dim']))
    elif meta['kind'] == 'node':
        model = NodePredictor(**kw)
    else:
        model = GraphPredictor(**kw, graph_pooling=(MeanEmbdPooling if op == 'mean' else SumEmbdPooling)(kw['in_dim']))
    model.load_state_dict(sd, strict=True)  # a reference checkpoint, as it is
    return model.eval()


def test_fixture_set_is_complete():
    assert dr.fixture_names() == dr.EXPECTED_FIXTURES and len(dr.EXPECTED_FIXTURES) == 11
    for name in dr.EXPECTED_FIXTURES:
        assert os.path.getsize(os.path.join(dr.GOLDEN, f'g26_decoder_{name}.npz')) < 400_000
        meta, sd, inputs, out = dr.load_fixture(name)
        kind, kw, op, rows = dr.CASES[name]
        assert (meta['kind'], meta['kw'], meta['op'], meta['rows']) == (kind, kw, op, rows)
        assert all(v.shape[0] == rows for v in inputs.values())


@pytest.mark.parametrize('name', dr.EXPECTED_FIXTURES)
def test_restatement_reproduces_the_recorded_outputs(name):
    meta, sd, inputs, out = dr.load_fixture(name)
    for dtype in (torch.float32, torch.float64):
        dr.close(dr.restate(meta, sd, inputs, dtype).float(), out, f'{name} {dtype}')


def test_reference_test_files_replay():
    """The reference's test_linkdecoder.py, test_nodedecoder.py and test_graphdecoder.py, every case (its own process: the replay aliases
    ``tgm`` to ``tgm_amd`` in ``sys.modules``).  Exit code 77: no reference checkout beside the repository."""
    r = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'replay_reference_decoders.py')], capture_output=True, text=True)
    if r.returncode == 77:
        pytest.skip('no reference checkout')
    assert r.returncode == 0 and 'all cases passed' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('name', dr.EXPECTED_FIXTURES)
def test_state_dict_keys_and_host_path(name):
    meta, sd, inputs, out = dr.load_fixture(name)
    model = build(meta, sd)
    assert list(model.state_dict()) == [k[2:] for k in meta['keys']]  # the reference's keys, in its order
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == dr.expected_keys(meta['kind'], meta['kw'], meta['op'])
    assert isinstance(model.model, torch.nn.Sequential) and isinstance(model.model[0], torch.nn.Linear) and isinstance(model.model[1], torch.nn.ReLU)
    for grad in (True, False):  # the torch path, with and without autograd
        with torch.set_grad_enabled(grad):
            got = model(*inputs.values())
        assert got.requires_grad == grad and got.shape == out.shape
        dr.close(got.detach(), out, f'{name} on the host')
        dr.close(got.detach(), dr.restate(meta, sd, inputs).float(), f'{name} against the restatement')


def test_import_paths_and_signatures():
    import tgm_amd.nn as nn_
    from tgm_amd.exceptions import BadAggregatorProtocolError, TGMError
    from tgm_amd.nn.decoder import GraphPredictor, LinkPredictor, NCNPredictor, NodePredictor  # noqa: F401
    from tgm_amd.nn.decoder.graphproppred import GraphPredictor as G2
    from tgm_amd.nn.decoder.linkproppred import LinkPredictor as L2
    from tgm_amd.nn.decoder.nodeproppred import NodePredictor as N2
    from tgm_amd.nn.modules import Aggregator, ConcatMerge, LearnableSumMerge, MeanEmbdPooling, SumEmbdPooling
    from tgm_amd.nn.modules.aggregation import ConcatMerge as C2

    assert (L2, N2, G2, C2) == (nn_.LinkPredictor, nn_.NodePredictor, nn_.GraphPredictor, ConcatMerge)
    assert issubclass(BadAggregatorProtocolError, TGMError)
    params = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]
    assert params(L2.__init__) == [('node_dim', inspect.Parameter.empty), ('out_dim', 1), ('nlayers', 2), ('hidden_dim', 64), ('merge_op', None)]
    assert params(N2.__init__) == [('in_dim', inspect.Parameter.empty), ('out_dim', 1), ('nlayers', 2), ('hidden_dim', 64)]
    assert params(G2.__init__) == [('in_dim', inspect.Parameter.empty), ('out_dim', 1), ('nlayers', 2), ('hidden_dim', 64), ('graph_pooling', None)]
    assert [n for n, _ in params(L2.forward)] == ['z_src', 'z_dst'] and [n for n, _ in params(N2.forward)] == ['z_node']
    assert [n for n, _ in params(G2.forward)] == ['z_nodes']
    assert [n for n, _ in params(L2.score_pairs)] == ['z', 'src_idx', 'dst_idx']
    assert [n for n, _ in params(L2.query_one_vs_many)] == ['z', 'src_idx', 'dst_idx', 'negatives']
    for op, width in ((ConcatMerge(6), 12), (LearnableSumMerge(6), 6), (MeanEmbdPooling(6), 6), (SumEmbdPooling(6), 6)):
        assert isinstance(op, Aggregator) and op.out_channels == width
    assert list(LearnableSumMerge(3).state_dict()) == ['lin_src.weight', 'lin_src.bias', 'lin_dst.weight', 'lin_dst.bias']
    ints = torch.arange(6).view(3, 2)
    cat = ConcatMerge(2)(ints, ints + 10)
    assert cat.dtype == torch.int64 and cat.tolist() == [[0, 1, 10, 11], [2, 3, 12, 13], [4, 5, 14, 15]]  # integers pass through unchanged
    assert isinstance(L2(4).merge, ConcatMerge) and isinstance(G2(4).graph_pooling, MeanEmbdPooling)
    assert len(L2(4, nlayers=1).model) == len(L2(4, nlayers=2).model) == 3 and len(N2(4, nlayers=4).model) == 7


def test_bad_protocol_error():
    from tgm_amd.exceptions import BadAggregatorProtocolError
    from tgm_amd.nn import GraphPredictor, LinkPredictor

    class NoWidth:
        def __call__(self, *a):
            return a[0]

    for make in (lambda: LinkPredictor(4, merge_op=NoWidth()), lambda: GraphPredictor(4, graph_pooling=NoWidth()), lambda: LinkPredictor(4, merge_op=3)):
        with pytest.raises(BadAggregatorProtocolError, match='Cannot validate .*: must implement __call__'):
            make()


@pytest.mark.parametrize('merge', ['concat', 'sum'])
def test_host_path_of_the_pair_methods_equals_the_per_positive_loop(merge):
    from tgm_amd.nn import LinkPredictor
    from tgm_amd.nn.modules import ConcatMerge, LearnableSumMerge

    torch.manual_seed(0)
    model = LinkPredictor(6, hidden_dim=9, merge_op=(ConcatMerge if merge == 'concat' else LearnableSumMerge)(6)).eval()
    g = torch.Generator().manual_seed(1)
    z = torch.randn(15, 6, generator=g)
    src, dst = torch.randint(0, 15, (5,), generator=g), torch.randint(0, 15, (5,), generator=g)
    fixed = torch.randint(0, 15, (5, 4), generator=g)
    ragged = [torch.randint(0, 15, (n,), generator=g) for n in (2, 0, 1, 7, 0)]
    with torch.no_grad():
        for idx in (torch.int64, torch.int32):
            many = model.query_one_vs_many(z, src.to(idx), dst.to(idx), fixed.to(idx))
            loop = dr.one_vs_many_loop(model, z, src, dst, list(fixed))
            assert tuple(many.shape) == (5, 5)
            for b in range(5):
                torch.testing.assert_close(many[b], loop[b], rtol=1e-6, atol=1e-6)
            lists = model.query_one_vs_many(z, src.to(idx), dst.to(idx), [n.to(idx) for n in ragged])
            loop = dr.one_vs_many_loop(model, z, src, dst, ragged)
            assert [t.numel() for t in lists] == [3, 1, 2, 8, 1]
            for b in range(5):
                torch.testing.assert_close(lists[b], loop[b], rtol=1e-6, atol=1e-6)
            torch.testing.assert_close(model.score_pairs(z, src.to(idx), dst.to(idx)), model(z[src], z[dst]), rtol=1e-6, atol=1e-6)
        assert model.query_one_vs_many(z, src[:0], dst[:0], []) == []
        with pytest.raises(ValueError):
            model.query_one_vs_many(z, src, dst[:4], fixed)
        with pytest.raises(ValueError):
            model.query_one_vs_many(z, src, dst, ragged[:3])
    assert model.score_pairs(z.requires_grad_(), src, dst).requires_grad
    model.check()  # nothing ran on a device: nothing to report


def test_abi_additions():
    from tgm_amd import _native

    lib = _native.load()
    for name in ('tgmx_decoder_pair_gemm', 'tgmx_decoder_score', 'tgmx_decoder_tail', 'tgmx_pool_rows', 'tgmx_pool_rows_scratch_floats', 'tgmx_decoder_row_mlp',
                 'tgmx_decoder_forward'):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.tgmx_abi_sizeof(27) == ctypes.sizeof(_native.DecoderFwd) > 0 and lib.tgmx_version() == 7
    assert ctypes.sizeof(_native.DecoderLayer) == 24 and _native.DECODER_MAX_LAYERS == 8
    assert _native.DECODER_FORM == {'rows': 0, 'pair': 1, 'table': 2} and _native.DECODER_POOL == {None: 0, 'mean': 1, 'sum': 2}
    assert lib.tgmx_pool_rows_scratch_floats(128, 7) == 0 and lib.tgmx_pool_rows_scratch_floats(129, 7) == 28  # two chunks of 7 doubles
