"""Decoder training without a GPU: the hand-written gradients (tests/decoders_bwd_restate.py) against float64 autograd of the restated
forward and against the reference's recorded gradients (tests/golden/g30_decoder_grad_*.npz), the ABI additions, the argument checks of the
new entry points, and the dispatch on the host."""
import ctypes
import os

import pytest
import torch

import decoders_bwd_restate as br
import decoders_restate as dr

# (kind, merge, constructor arguments): the heads of tests/test_decoders_gpu.py's CONFIGS and two NodePredictors
HEADS = {
    'concat': ('link', 'concat', dict()),
    'concat-deep-out3': ('link', 'concat', dict(nlayers=3, out_dim=3)),
    'concat-out20': ('link', 'concat', dict(out_dim=20)),
    'sum': ('link', 'sum', dict()),
    'sum-deep': ('link', 'sum', dict(nlayers=3)),
    'node': ('node', None, dict(out_dim=2)),
}


def make_head(kind, op, kw, D=24, H=32, seed=0):
    from tgm_amd.nn import LinkPredictor, NodePredictor
    from tgm_amd.nn.modules import ConcatMerge, LearnableSumMerge

    torch.manual_seed(seed)
    if kind == 'link':
        return LinkPredictor(D, hidden_dim=H, merge_op=(ConcatMerge if op == 'concat' else LearnableSumMerge)(D), **kw)
    return NodePredictor(D, hidden_dim=H, **kw)


@pytest.mark.parametrize('name', sorted(HEADS))
def test_restatement_equals_float64_autograd(name):
    kind, op, kw = HEADS[name]
    model = make_head(kind, op, kw)
    sd = {k: v.detach().double().requires_grad_() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    R, D = 30, 24
    inputs = {k: torch.randn(R, D, generator=g, dtype=torch.float64).requires_grad_() for k in (('z_src', 'z_dst') if kind == 'link' else ('z',))}
    out = dr.link(sd, op, *inputs.values()) if kind == 'link' else dr.node(sd, inputs['z'])
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    got = br.head_grads(sd, kind, op, {k: v.detach() for k, v in inputs.items()}, dout)
    want = {**{k: v.grad for k, v in sd.items()}, **{k: v.grad for k, v in inputs.items()}}
    assert set(got) == set(want)
    for k, (val, bound) in got.items():
        assert dr.rel_err(val, want[k]) <= 1e-12, (name, k)
        assert (bound >= 0).all() and torch.isfinite(bound).all()
    if kind == 'link':  # the table form: the same pairs through indices into one table
        z = torch.randn(17, D, generator=g, dtype=torch.float64).requires_grad_()
        ia, ib = torch.randint(0, 17, (R,), generator=g), torch.randint(0, 17, (R,), generator=g)
        for p in sd.values():
            p.grad = None
        dr.link(sd, op, z[ia], z[ib]).backward(dout)
        got = br.head_grads(sd, kind, op, {'z': z.detach()}, dout, idx=(ia, ib))
        for k, (val, _) in got.items():
            assert dr.rel_err(val, z.grad if k == 'z' else sd[k].grad) <= 1e-12, (name, k, 'table')


def test_grad_fixture_set_is_complete():
    assert br.grad_fixture_names() == br.EXPECTED_GRAD_FIXTURES and len(br.EXPECTED_GRAD_FIXTURES) == 4
    for name in br.EXPECTED_GRAD_FIXTURES:
        assert os.path.getsize(os.path.join(dr.GOLDEN, f'g30_decoder_grad_{name}.npz')) < 500_000
        meta, sd, inputs, dout, grads = br.load_grad_fixture(name)
        kind, kw, op, rows = br.GRAD_CASES[name]
        assert (meta['kind'], meta['kw'], meta['op'], meta['rows']) == (kind, kw, op, rows)
        assert set(grads) == set(sd) | set(inputs) and all(grads[k].shape == v.shape for k, v in {**sd, **inputs}.items())


@pytest.mark.parametrize('name', br.EXPECTED_GRAD_FIXTURES)
def test_restatement_meets_the_recorded_gradients(name):
    meta, sd, inputs, dout, grads = br.load_grad_fixture(name)
    for k, (val, _) in br.head_grads(sd, meta['kind'], meta['op'], inputs, dout).items():
        dr.close(val.float(), grads[k], f'{name} {k}')


def test_chain_lengths_follow_the_launch_code():
    assert [br.tail_bwd_rpb(R) for R in (1, 200, 1024, 1025, 100_000)] == [4, 4, 4, 8, 392]
    assert br.tail_bwd_chain(200) == 1 + 3 + 50
    assert br.sgemm_tn_chain(30, 32, 24) == 32 + 1 and br.sgemm_tn_chain(600, 100, 100) == 64 + 10
    assert br.colsum_chain(400) == 58 + 7
    assert [br.scatter_chain(c, 10_000) for c in (0, 64, 65, 2048, 2049)] == [1, 64, 21, 516, 256 + 4 + 2 + 2]


def test_abi_additions():
    from tgm_amd import _native

    lib = _native.load()
    for name in ('tgmx_decoder_forward_save', 'tgmx_decoder_backward', 'tgmx_decoder_backward_workspace_bytes', 'tgmx_decoder_tail_bwd',
                 'tgmx_decoder_tail_bwd_workspace_floats', 'tgmx_decoder_scatter', 'tgmx_decoder_scatter_workspace_bytes', 'tgmx_decoder_drop_rows'):  # fmt: skip
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.tgmx_abi_sizeof(30) == ctypes.sizeof(_native.DecoderTrain) > ctypes.sizeof(_native.DecoderFwd) and lib.tgmx_version() == 7
    assert lib.tgmx_abi_sizeof(27) == ctypes.sizeof(_native.DecoderFwd) and lib.tgmx_abi_sizeof(31) == 0
    assert ctypes.sizeof(_native.DropJob) == 40
    assert lib.tgmx_decoder_tail_bwd_workspace_floats(200, 100, 1) == 50 * 101 and lib.tgmx_decoder_tail_bwd_workspace_floats(0, 100, 1) == 0
    assert lib.tgmx_decoder_scatter_workspace_bytes(400, 600, 100) > 0 and lib.tgmx_decoder_scatter_workspace_bytes(1 << 30, 600, 100) == 0


def test_new_entry_points_reject_null_pointers_and_bad_sizes():
    """Every check below fails before anything is launched: no device is needed."""
    from tgm_amd import _native

    lib = _native.load()
    E_INVALID = lib.tgmx_decoder_forward_save(None, None)
    assert E_INVALID != 0 and lib.tgmx_decoder_backward(None, None) == E_INVALID and lib.tgmx_decoder_backward_workspace_bytes(None) == 0
    x = 0x1000  # (never dereferenced: the calls return before any launch)
    assert lib.tgmx_decoder_tail_bwd(None, 1, x, 8, 4, 8, x, 1, 1, x, 8, x, x, x, 1 << 20, None) == E_INVALID  # no upstream gradient
    assert lib.tgmx_decoder_tail_bwd(x, 1, x, 4, 4, 8, x, 1, 1, x, 8, x, x, x, 1 << 20, None) == E_INVALID  # ldx < K
    assert lib.tgmx_decoder_tail_bwd(x, 1, x, 8, 4, 8, x, 1, 1, x, 8, x, x, x, 3, None) == E_INVALID  # workspace too small
    assert lib.tgmx_decoder_tail_bwd(x, 1, x, 8, 4, 8, x, 1, 1, x, 8, x, x, None, 0, None) == E_INVALID  # no workspace for the sums
    assert lib.tgmx_decoder_tail_bwd(x, 17, x, 8, 4, 8, x, 17, 1, x, 8, x, x, x, 1 << 20, None) == _native.E_UNSUPPORTED  # 17 outputs
    assert b'out_dim=17' in lib.tgmx_last_error()
    assert lib.tgmx_decoder_tail_bwd(x, 1, x, 8, 0, 8, x, 1, 1, x, 8, x, x, None, 0, None) == 0  # R = 0: nothing to do
    assert lib.tgmx_decoder_scatter(x, 4, 3, 8, x, x, 0, 5, x, x, 1 << 20, None) == E_INVALID  # lddh < H
    assert lib.tgmx_decoder_scatter(None, 8, 3, 8, x, x, 0, 5, x, x, 1 << 20, None) == E_INVALID
    assert lib.tgmx_decoder_scatter(x, 8, 3, 8, x, x, 0, 5, x, x, 16, None) == E_INVALID  # workspace too small
    assert lib.tgmx_decoder_scatter(x, 8, 1 << 30, 8, x, x, 0, 5, x, x, 1 << 20, None) == E_INVALID
    assert lib.tgmx_decoder_drop_rows(None, x, 0, 5, 3, None, 1, None) == E_INVALID and lib.tgmx_decoder_drop_rows(x, x, 0, 5, 3, None, 99, None) == E_INVALID
    t = _native.DecoderTrain()
    assert lib.tgmx_decoder_forward_save(ctypes.byref(t), None) == E_INVALID and b'layers' in lib.tgmx_last_error()  # no layers
    t.fwd.num_layers, t.fwd.form, t.fwd.D, t.fwd.R, t.fwd.lda1 = 1, _native.DECODER_FORM['rows'], 8, 4, 8
    t.fwd.layers[0].w, t.fwd.layers[0].in_, t.fwd.layers[0].out = x, 8, 1
    assert lib.tgmx_decoder_forward_save(ctypes.byref(t), None) == E_INVALID  # no operand
    t.fwd.a1, t.fwd.out = x, x
    assert lib.tgmx_decoder_backward(ctypes.byref(t), None) == E_INVALID and b'upstream' in lib.tgmx_last_error()
    t.dout, t.lddout, t.d_a2 = x, 1, x
    assert lib.tgmx_decoder_backward(ctypes.byref(t), None) == E_INVALID and b'no merge stage' in lib.tgmx_last_error()
    t.d_a2, t.d_a1 = None, x
    assert lib.tgmx_decoder_backward_workspace_bytes(ctypes.byref(t)) > 0
    assert lib.tgmx_decoder_backward(ctypes.byref(t), None) == E_INVALID and b'workspace too small' in lib.tgmx_last_error()
    t.fwd.pool = 1
    assert lib.tgmx_decoder_backward(ctypes.byref(t), None) == E_INVALID and b'pooling' in lib.tgmx_last_error()


def test_host_tensors_with_gradients_take_the_torch_path(monkeypatch):
    from tgm_amd.nn import _decoder_train
    from tgm_amd.nn._decoder_train import DecoderFunction

    assert _decoder_train.mode() == 'native'
    monkeypatch.setenv('TGMX_DECODER_BWD', 'py')
    assert _decoder_train.mode() == 'py'
    monkeypatch.delenv('TGMX_DECODER_BWD')
    g = torch.Generator().manual_seed(2)
    for name, (kind, op, kw) in HEADS.items():
        model = make_head(kind, op, kw).train()
        zs = [torch.randn(9, 24, generator=g).requires_grad_() for _ in range(2 if kind == 'link' else 1)]
        assert not model._trainable(*zs)
        out = model(*zs)
        assert out.requires_grad and DecoderFunction.__name__ not in type(out.grad_fn).__name__
        out.sum().backward()
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        dout = torch.ones(out.shape)
        inputs = dict(zip(('z_src', 'z_dst') if kind == 'link' else ('z',), (z.detach() for z in zs)))
        for k, (val, _) in br.head_grads(sd, kind, op, inputs, dout).items():
            got = dict(model.named_parameters())[k].grad if k in sd else zs[list(inputs).index(k)].grad
            dr.close(got, val.float(), f'{name} {k} on the host')
        if kind == 'link':
            z = zs[0]
            idx = torch.arange(9)
            assert 'DecoderFunction' not in type(model.score_pairs(z, idx, idx.flip(0)).grad_fn).__name__
