"""NCNPredictor training at k = 8 on the native path (csrc/ncn8_bwd.hip): gradients against float64 autograd through tests/ncn8_restate.py,
the coefficient-slab kernel alone, bits (two runs, LDS against workspace rows, one call against one launch at a time), slab sizes, and the
shape of a training step.  The bar is the project's gradient bar, 1e-4 of each gradient's largest entry.  Before the k = 8 backward existed
``forward`` under gradients took the composed path: ``type(out.grad_fn)`` was not ``NcnFunction``'s."""
import functools

import pytest
import torch

from golden_util import load
import ncn8_restate as n8
import ncn_restate as nr
from test_ncn_cpu import CN_BAR, fixture_inputs
from test_ncn_gpu import DEV, dev, model_from_fixture

pytestmark = pytest.mark.gpu
PARAMS = [f'xsmlp.{layer}.{p}' for layer in (0, 2) for p in ('weight', 'bias')]


def setup(name, dup='last', drop=0):
    """(meta, model in training mode, device inputs without the last ``drop`` pairs)"""
    meta, a = load(name)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    B = tar.shape[1] - drop
    m, _ = model_from_fixture(meta, a, duplicate_targets=dup)
    return meta, m.train(), [dev(t) for t in (x, ei, tar[:, :B].contiguous(), lu, None if et is None else et[:B])]


def grads(m, x, ei, tar, lu, et, x_grad=True):
    """(out, [dx, d w1, d b1, d w2, d b2], is the grad_fn NcnFunction's) with the loss sum(out * linspace(-1, 1))"""
    m.zero_grad(set_to_none=True)
    xd = x.clone().requires_grad_(x_grad)
    out = m(xd, ei, tar, lu, et)
    (out * torch.linspace(-1, 1, out.numel(), dtype=torch.float64).to(DEV).float()).sum().backward()
    return out.detach(), [xd.grad] + [m.get_parameter(n).grad for n in PARAMS], 'NcnFunction' in type(out.grad_fn).__name__


@functools.lru_cache(maxsize=None)
def ref64(name, dup='last', drop=0):
    """float64 autograd through the dense restatement: [dx, d w1, d b1, d w2, d b2]"""
    meta, a = load(name)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    B = tar.shape[1] - drop
    sd = {n: v.double().requires_grad_(True) for n, v in nr.fixture_state_dict(meta, a).items()}
    x64 = x.double().requires_grad_(True)
    out = n8.forward(sd, x64, ei, tar[:, :B], lu, None if et is None else et[:B], duplicate_targets=dup)
    (out * torch.linspace(-1, 1, out.numel(), dtype=torch.float64)).sum().backward()
    return [x64.grad] + [sd[n].grad for n in PARAMS]


def excess(got, ref, floor=0.0):
    """max |got - ref| over the bar, 1e-4 of ref's largest entry: <= 1 passes.  ``floor``: d b2 = sum of the loss weights, which linspace(-1, 1)
    makes zero up to rounding, so its float64 value is noise and 1e-4 of it is no bar; B float32 roundings of weights below 1 (B 2^-24) is."""
    ref = ref.to(got.device).double()
    if ref.numel() == 0:
        return 0.0
    return float((got.double() - ref).abs().max()) / max(1e-4 * float(ref.abs().max()), floor)


def raw_dx(m, x, ei, tar, lu, et, dxs, slab=0, force=0):
    """``tgmx_ncn8_dx`` itself on a given dxs [B, 8 C]"""
    from tgm_amd import _native
    from tgm_amd.nn.ncn import adjacency

    lib, (N, C), B = _native.load(), x.shape, tar.shape[1]
    adj, last = adjacency(N, ei), last_marks(tar, N)
    need = lib.tgmx_ncn8_dx_workspace_bytes(N, B, C, slab, force)
    ws, dx = torch.empty(need, dtype=torch.uint8, device=DEV), torch.full((N, C), float('nan'), device=DEV)
    _native.check(lib.tgmx_ncn8_dx(x.data_ptr(), N, C, adj.indptr.data_ptr(), adj.cols.data_ptr(), tar.data_ptr(), 1, B, B, _native.ptr(lu), _native.ptr(et),
                                   None if m.duplicate_targets == 'all' else last.data_ptr(), dxs.data_ptr(), 8 * C, dx.data_ptr(), slab, ws.data_ptr(), need,
                                   force, _native.stream_ptr()), 'tgmx_ncn8_dx')  # fmt: skip
    return dx


def last_marks(tar, N):
    last = torch.full((2 * N,), -1, dtype=torch.int32)
    for r, (i, j) in enumerate(tar.t().tolist()):
        last[i], last[N + j] = r, r
    return last.to(DEV)


GRAD_CASES = ['triangle_decay', 'selfloop_plain', 'samepair_decay', 'onevsmany_decay', 'hub', 'width_c1', 'width_c65', 'width_c300', 'wide_n7681']


@pytest.mark.parametrize('dup', ['last', 'all'])
@pytest.mark.parametrize('name', ['g34_ncn8_' + c for c in GRAD_CASES])
def test_gradients_against_float64(name, dup):
    _, m, inp = setup(name, dup)
    out, got, native = grads(m, *inp)
    assert native and m.xslin.weight.grad is None and m.xslin.bias.grad is None
    with torch.no_grad():
        assert torch.equal(out, m(*inp))  # the saving forward is the no-grad call
    for what, g, r in zip(['x'] + PARAMS, got, ref64(name, dup)):
        e = excess(g, r, inp[2].shape[1] * 2.0**-24 if what == 'xsmlp.2.bias' else 0.0)
        print(f'{name} {dup} d {what}: {e:.3f} of the bar')
        assert e <= 1.0, what


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_selfloop_plain', 'g34_ncn8_hub'])
def test_coefficient_slab_kernel(name):
    from tgm_amd import _native
    from tgm_amd.nn.ncn import adjacency

    meta, m, (x, ei, tar, lu, et) = setup(name)
    N, B, C = meta['N'], tar.shape[1], meta['C']
    first, P, ldT = 2, B - 3, (N + 63) // 64 * 64  # a slab that starts and ends inside the batch
    adj, last = adjacency(N, ei), last_marks(tar, N)
    T = torch.full((8 * P, ldT), float('nan'), device=DEV)
    _native.check(_native.load().tgmx_ncn8_coef(N, adj.indptr.data_ptr(), adj.cols.data_ptr(), tar.data_ptr(), 1, B, B, _native.ptr(lu), _native.ptr(et),
                                                last.data_ptr(), first, P, T.data_ptr(), ldT, None, 0, 0, _native.stream_ptr()), 'tgmx_ncn8_coef')  # fmt: skip
    T = T.cpu().double()
    assert not T.isnan().any() and not T[0::8].any() and not T[:, N:].any()  # every element stored; rows 8 s and the pad columns zero
    co = n8.coefficients(N, ei.cpu(), tar.cpu())
    with torch.no_grad():
        cn = m.get_cn_emb(x, ei, tar, (lu, et)).cpu().double()
    for b, blk in enumerate(n8.BLOCKS):
        rows = T[b + 1 :: 8, :N]
        if lu is None:
            assert torch.equal(rows, co[blk][first : first + P]), blk  # integers below 2^24: exact
        else:
            assert nr.rel_err(rows @ x.cpu().double(), cn[first : first + P, b * C : (b + 1) * C]) < CN_BAR, blk
    idle = ~(nr.kept_rows(tar[0].cpu(), 'last') & nr.kept_rows(tar[1].cpu(), 'last'))[first : first + P]
    assert not T.view(P, 8 * ldT)[idle].any() and T.view(P, 8 * ldT)[~idle].any()


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_hub'])
def test_bits_and_slabs(name, monkeypatch):
    meta, m, inp = setup(name, drop=1)  # B = 8 / 32: not a multiple of 3
    x, ei, tar, lu, et = inp
    B, ref = tar.shape[1], ref64(name, 'last', 1)
    assert B % 3
    base = grads(m, *inp)[1]
    same = lambda g: all(torch.equal(p, q) for p, q in zip(g, base))
    assert same(grads(m, *inp)[1]) and excess(base[0], ref[0]) <= 1.0  # two runs
    monkeypatch.setenv('TGMX_NCN_BWD', 'py')
    out, g, native = grads(m, *inp)
    assert native and same(g)  # one launch per ctypes call: the same bits
    monkeypatch.delenv('TGMX_NCN_BWD')
    for slab in (1, 3):  # other slab sizes group dx's sum differently: within the bar, not bit for bit
        monkeypatch.setattr(m, '_slab_pairs', slab)
        assert excess(grads(m, *inp)[1][0], ref[0]) <= 1.0
    dxs = torch.randn(B, 8 * meta['C'], generator=torch.Generator().manual_seed(B)).to(DEV)
    lds = raw_dx(m, *inp, dxs)
    assert lds.any() and torch.equal(lds, raw_dx(m, *inp, dxs)) and torch.equal(lds, raw_dx(m, *inp, dxs, force=1))  # LDS rows, workspace rows
    assert excess(raw_dx(m, *inp, dxs, slab=3, force=1), lds) <= 1.0
    # more pairs than resident workspace regions (256): a region serves several pairs, each finding it as the one before left it
    reps = -(-600 // B)
    monkeypatch.setattr(m, 'duplicate_targets', 'all')
    one = raw_dx(m, *inp, dxs, force=1)
    many = raw_dx(m, x, ei, tar.repeat(1, reps), lu, None if et is None else et.repeat(reps), dxs.repeat(reps, 1), force=1)
    assert excess(many, reps * one) <= 1.0


def test_the_shape_of_a_training_step(monkeypatch):
    from tgm_amd.nn.ncn import adjacency

    meta, m, (x, ei, tar, lu, et) = setup('g34_ncn8_triangle_decay')
    N, adj = meta['N'], adjacency(meta['N'], ei)
    bad = tar.clone()
    bad[0, 2], bad[1, 5] = N, -1  # a target outside the node table: no gradient, never dereferenced

    def step(targets):  # a positive and a negative call through one prepared adjacency, one backward
        m.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        pos, neg = m(xd, adj, targets, lu, et), m(xd, adj, targets.flip(0), lu, et)
        (pos.sum() - 0.5 * neg.sum()).backward()
        return [xd.grad] + [m.get_parameter(n).grad for n in PARAMS], 'NcnFunction' in type(pos.grad_fn).__name__

    native = {k: step(t) for k, t in (('tar', tar), ('bad', bad))}
    monkeypatch.setenv('TGMX_NCN_BWD', 'torch')
    for k, t in (('tar', tar), ('bad', bad)):
        composed, fn = step(t)
        assert native[k][1] and not fn
        assert all(excess(g, r) <= 1.0 for g, r in zip(native[k][0], composed)), k
    monkeypatch.delenv('TGMX_NCN_BWD')
    # requires_grad subsets: the remaining gradients keep their bits
    base = grads(m, x, ei, tar, lu, et)[1]
    frozen_x = grads(m, x, ei, tar, lu, et, x_grad=False)[1]
    assert frozen_x[0] is None and all(torch.equal(p, q) for p, q in zip(frozen_x[1:], base[1:]))
    m.xsmlp[0].weight.requires_grad_(False)
    frozen_w = grads(m, x, ei, tar, lu, et)[1]
    m.xsmlp[0].weight.requires_grad_(True)
    assert frozen_w[1] is None and all(torch.equal(p, q) for p, q in zip(frozen_w[:1] + frozen_w[2:], base[:1] + base[2:]))
    out, empty, fn = grads(m, x, ei, tar[:, :0], lu, et[:0])  # B = 0: every gradient asked for is zero
    assert fn and out.shape == (0,) and all(g.shape == b.shape and not g.any() for g, b in zip(empty, base))
